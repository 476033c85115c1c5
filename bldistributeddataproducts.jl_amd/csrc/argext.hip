// argext.hip — fqavfunc argmax / argmin of Float32 windows (gfx950): where in
// each F x T block of the reduce the extreme lies, the other half of Julia's
// findmax / findmin.
//
// The block of output (c', i, t') is the reduce's: F selected channels by T
// selected spectra, numbered off = k + F * tt (0-based, channel fastest: the
// order of reshape(A, (F, :, ni, T, :))).  The result is the smallest off of a
// NaN when the block holds one, else the smallest off among the elements that
// are greatest (argmax) or least (argmin) under isless (-0.0 < 0.0).
//
// Every element becomes a key whose unsigned order is the rule: f2key's image
// of the float (stats.hip), inverted for argmin, and 0xffffffff for a NaN of
// either sign (above every other key in both cases).  What is reduced is the
// pair (key, off) as one 64-bit word, key in the high half and ~off in the low
// one: the maximum of the words is the greatest key and, among equal keys, the
// smallest off.  max is associative and commutative, so the result is the same
// whatever lanes, waves or time slices share a block.  A lane walks its own
// elements in increasing off, so there it keeps (key, off) apart and replaces
// them on a strictly greater key only.
//
// The value output is the winning element's bit pattern: rebuilt from the key,
// which is a bijection of the bits, except for a NaN, whose payload the
// canonical key dropped; that one element is read again.
//
//   k_arg_lanes  (F <= 1024)  the 1 .. 64 lanes of a wave that share a block
//                stream its T rows, <= 16 elements a lane a row (float4 loads at
//                any dword alignment on unit-step windows with F % 4 == 0, else
//                one dword per element); the next row's loads are issued before
//                the current row's compares, and where the rows are not split
//                a lane with one item a row (every F <= 256 with float4 loads,
//                F <= 64 with dwords) takes 4 (dwords: 16) rows a batch, the
//                next batch in flight behind it.  The lanes meet once, by
//                xor-shuffles of the pair.  With ts > 1 time slices a workgroup
//                holds kBlock / (lanes * ts) blocks and slice s takes rows s,
//                s + ts, ...; the slices meet once through LDS (blocks with long
//                T and too few outputs to fill the GPU).
//   k_arg_block  (F > 1024)   one workgroup per block, rows streamed; the waves
//                meet once through LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bldp_impl.h"

namespace bldp {
namespace {

constexpr int kBlock = 256;  // 4 waves of 64
// a float4 on any dword boundary (kernels.hip f4u)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int64_t kLaneMaxF = 1024;      // k_arg_lanes: 64 lanes x 16 values a row
constexpr uint32_t kNanKey = 0xffffffffu;  // above every other key, argmax and argmin
typedef unsigned long long u64;

__device__ __forceinline__ float4 ld4(const float *p) {
  const f4u v = *reinterpret_cast<const f4u *>(p);
  return make_float4(v.x, v.y, v.z, v.w);
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

// Block g of bank blockIdx.y: its first element and its output index; false past the end.
__device__ __forceinline__ bool arg_group(const RedArgs &a, int64_t g, const float *&p,
                                          int64_t &o) {
  if (g >= a.nco * a.ni * a.nto) return false;
  int64_t co, r, i, t;
  divmod(g, a.nco, r, co);
  divmod(r, a.ni, t, i);
  const int64_t b = blockIdx.y;
  p = a.in[b] + a.in_off + co * a.F * a.in_cs + i * a.in_ld_i + t * a.T * a.in_ld_t;
  o = b * a.out_bank + co + i * a.out_ld_i + t * a.out_ld_t;
  return true;
}

// The canonical key: isless order as unsigned order (stats.hip f2key), inverted
// for argmin (inv = 0xffffffff, else 0); every NaN is the greatest.  Keys of
// numbers lie in [0x007fffff, 0xff800000] either way, so 0 is below them all.
__device__ __forceinline__ uint32_t arg_key(float x, uint32_t inv) {
  const uint32_t u = __float_as_uint(x);
  const uint32_t k = ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) ^ inv;
  return x != x ? kNanKey : k;
}

__device__ __forceinline__ u64 arg_pair(uint32_t key, uint32_t off) {
  return ((u64)key << 32) | (uint32_t)~off;
}

__device__ __forceinline__ u64 pair_max(u64 x, u64 y) { return x > y ? x : y; }

// Store the block's result: the offset, and the winner's bits when asked.
__device__ __forceinline__ void arg_store(const ArgArgs &a, const float *p, int64_t o, u64 best) {
  const uint32_t key = (uint32_t)(best >> 32), off = ~(uint32_t)best;
  a.idx[o] = off;
  if (!a.r.out) return;
  if (key != kNanKey) {
    const uint32_t k = key ^ a.inv;
    a.r.out[o] = __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  } else {  // the first NaN's own payload
    const uint32_t F = (uint32_t)a.r.F, tt = off / F, k = off - tt * F;
    a.r.out[o] = p[(int64_t)k * a.r.in_cs + (int64_t)tt * a.r.in_ld_t];
  }
}

// MR: a lane has one item (a float4 or a value) of a row, and its register
// slots hold that item of NS successive rows of its slice instead of NS items
// of one row: NS rows' loads in flight, and the next NS behind them.
template <int LPG, bool VEC, bool MR>
__global__ __launch_bounds__(kBlock) void k_arg_lanes(const ArgArgs a) {
  __shared__ u64 sh[kBlock];  // the slices' pairs (ts > 1)
  const RedArgs &r = a.r;
  constexpr int GW = kBlock / LPG;          // lane groups of a workgroup: blocks x slices
  constexpr int NS = VEC ? 4 : 16;          // register slots of a lane
  constexpr int EP = VEC ? 4 : 1;           // elements of a slot
  const int tl = r.tsub_log2;               // log2 of the time slices, 2^tl <= GW
  const int TS = 1 << tl, G = GW >> tl;     // time slices; blocks of a workgroup
  const int lg = threadIdx.x % LPG;
  const int gi = (threadIdx.x / LPG) & (G - 1);
  const uint32_t sl = (threadIdx.x / LPG) >> (__builtin_ctz(GW) - tl);
  const int64_t tile = xcd_order(blockIdx.x, gridDim.x, r.xcd_lg);
  const float *p = nullptr;
  int64_t o = 0;
  const bool ok = arg_group(r, tile * G + gi, p, o);
  const int F = (int)r.F;
  const uint32_t T = ok ? (uint32_t)r.T : 0u;
  const uint32_t inv = a.inv;
  // slot s of the batch that starts at row tt: item it(s) of row row(s, tt)
  auto it = [&](int s) { return MR ? lg : lg + s * LPG; };
  auto row = [&](int s, uint32_t tt) { return MR ? tt + (uint32_t)(s * TS) : tt; };
  auto has = [&](int s, uint32_t tt) { return EP * it(s) < F && (!MR || row(s, tt) < T); };
  auto load = [&](float *d, uint32_t tt) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (has(s, tt)) {
        const float *q = p + (int64_t)row(s, tt) * r.in_ld_t;
        if (VEC) {
          const float4 x = ld4(q + 4 * it(s));
          d[4 * s] = x.x, d[4 * s + 1] = x.y, d[4 * s + 2] = x.z, d[4 * s + 3] = x.w;
        } else {
          d[s] = q[(int64_t)it(s) * r.in_cs];
        }
      }
  };
  const uint32_t step = MR ? NS * TS : TS;  // rows between a slice's batches
  uint32_t bk = 0, boff = 0;  // this lane's best so far (0: none yet)
  float v[16] = {}, nx[16] = {};
  if (sl < T) load(v, sl);
#pragma unroll 2
  for (uint32_t tt = sl; tt < T; tt += step) {
    if (tt + step < T) load(nx, tt + step);  // in flight under this batch's compares
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (has(s, tt)) {  // (slots in increasing offset: a strictly greater key only)
        const uint32_t base = (uint32_t)F * row(s, tt) + (uint32_t)(EP * it(s));
#pragma unroll
        for (int c = 0; c < EP; ++c) {
          const uint32_t key = arg_key(v[EP * s + c], inv);
          if (key > bk) bk = key, boff = base + c;
        }
      }
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = nx[u];
  }
  u64 best = arg_pair(bk, boff);
#pragma unroll
  for (int w = LPG / 2; w >= 1; w /= 2) best = pair_max(best, __shfl_xor(best, w, 64));
  if (TS > 1) {  // (uniform)
    if (lg == 0) sh[gi + G * sl] = best;
    __syncthreads();
    if (sl == 0 && lg == 0)
      for (int s = 1; s < TS; ++s) best = pair_max(best, sh[gi + G * s]);
  }
  if (ok && sl == 0 && lg == 0) arg_store(a, p, o, best);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_arg_block(const ArgArgs a) {
  __shared__ u64 sh[kBlock / 64];
  const RedArgs &r = a.r;
  const uint32_t tid = threadIdx.x;
  const float *p = nullptr;
  int64_t o = 0;
  if (!arg_group(r, blockIdx.x, p, o)) return;  // (uniform)
  const uint32_t F = (uint32_t)r.F, T = (uint32_t)r.T;
  const uint32_t n = VEC ? F / 4 : F;  // items of a row: float4s or values
  const uint32_t inv = a.inv;
  uint32_t bk = 0, boff = 0;
  auto take = [&](float x, uint32_t off) {
    const uint32_t key = arg_key(x, inv);
    if (key > bk) bk = key, boff = off;
  };
  for (uint32_t tt = 0; tt < T; ++tt) {
    const float *q = p + (int64_t)tt * r.in_ld_t;
    const uint32_t base = F * tt;
#pragma unroll 4
    for (uint32_t k = tid; k < n; k += kBlock) {
      if (VEC) {
        const float4 x = ld4(q + 4 * (int64_t)k);
        take(x.x, base + 4 * k), take(x.y, base + 4 * k + 1);
        take(x.z, base + 4 * k + 2), take(x.w, base + 4 * k + 3);
      } else {
        take(q[(int64_t)k * r.in_cs], base + k);
      }
    }
  }
  u64 best = arg_pair(bk, boff);
#pragma unroll
  for (int w = 32; w >= 1; w /= 2) best = pair_max(best, __shfl_xor(best, w, 64));
  if ((tid & 63) == 0) sh[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) best = pair_max(best, sh[w]);
    arg_store(a, p, o, best);
  }
}

// Rows between which a column's blocks lie, for the per-XCD tile order: the
// bounds of kernels.hip xcd_order_pays for the kernels that stream T rows
// (k_reduce_row) and for those that read one (k_reduce_vec: always).
constexpr int kXcdMinT = 8;
constexpr int64_t kXcdMinPitch = (int64_t)4 << 20, kXcdMaxPitch = (int64_t)128 << 20;

}  // namespace

int plan_argext(ArgArgs &aa, bool words, int num_cus, int xcd_lg, Plan *pp) {
  RedArgs &a = aa.r;
  Plan p{};
  const int64_t F = a.F, T = a.T;
  p.nout = a.nco * a.ni * a.nto;
  a.ts = 1;
  a.tpb = 1;
  a.tsub_log2 = 0;
  a.rsplit = 1;
  a.bpack = 0;
  a.st_plain = 1;
  a.vec_out = 0;
  a.nchunk = 1;
  a.rows_per_chunk = T;
  a.blocks_c = 1;
  a.div = 1.0f;
  a.xcd_lg = 0;
  const bool vec = words && F % 4 == 0;  // float4 loads
  const int64_t items = vec ? F / 4 : F;
  int64_t per_lane;  // items a lane takes of a row
  if (F <= kLaneMaxF) {
    int lpg = 1;
    while (lpg < 64 && lpg < items) lpg *= 2;
    // Blocks with long T and too few outputs to fill the GPU (4 waves a SIMD):
    // T over the time slices of a workgroup, 16 rows a slice at least.
    const int64_t waves = (p.nout * a.nbank * lpg + 63) / 64, want = (int64_t)num_cus * 16;
    int ts = 1;
    while (2 * ts * lpg <= kBlock && T / (2 * ts) >= 16 && waves * ts < want) ts *= 2;
    p.path = ts > 1 ? ARGEXT_LANES_TSPLIT : ARGEXT_LANES;
    p.lpg = lpg;
    a.ts = ts;
    while ((1 << a.tsub_log2) < ts) ++a.tsub_log2;
    const int64_t g = kBlock / (lpg * ts);
    a.ntiles = (p.nout + g - 1) / g;
    per_lane = (items + lpg - 1) / lpg;
    const int64_t pitch = 4 * a.in_ld_t;
    if (ts == 1 && (T == 1 || (T >= kXcdMinT && pitch >= kXcdMinPitch && pitch <= kXcdMaxPitch)))
      a.xcd_lg = xcd_lg;
  } else {
    p.path = ARGEXT_BLOCK;
    p.lpg = kBlock;
    a.ntiles = p.nout;
    per_lane = (items + kBlock - 1) / kBlock;
  }
  a.k4 = vec ? (int32_t)std::min<int64_t>(per_lane, INT32_MAX) : 0;
  if (a.ntiles > INT32_MAX)
    return set_error(BLDP_EINVAL, "argext: %lld blocks of %lld x %lld are too many for one launch",
                     (long long)p.nout, (long long)F, (long long)T);
  p.grid = a.ntiles;
  p.ws_bytes = 0;
  *pp = p;
  return BLDP_OK;
}

hipError_t launch_argext(const ArgArgs &a, const Plan &p, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  const dim3 grid((unsigned)p.grid, (unsigned)a.r.nbank);
  const bool vec = a.r.k4 != 0;
  // A lane with one item a row batches rows where there is more than one.  Not
  // in the time-split form: on one 0001 bank (F = 8, T = 1024, 4 slices) the
  // batches measured 0.405 ms against 0.317 ms a row at a time; unsplit, the
  // 0002 band at F = 64, T = 16 went from 0.134 to 0.123 ms (MI355X).
  const bool mr = a.r.ts == 1 && a.r.T > 1 && (vec ? a.r.F / 4 : a.r.F) <= p.lpg;
#define BLDP_ARG_LANES(N)                                                                  \
  case N:                                                                                  \
    hipLaunchKernelGGL((vec ? (mr ? k_arg_lanes<N, true, true> : k_arg_lanes<N, true, false>) \
                            : (mr ? k_arg_lanes<N, false, true> : k_arg_lanes<N, false, false>)), \
                       grid, dim3(kBlock), 0, s, a);                                       \
    return hipGetLastError();
  switch (p.path) {
    case ARGEXT_LANES:
    case ARGEXT_LANES_TSPLIT:
      switch (p.lpg) {
        BLDP_ARG_LANES(1)
        BLDP_ARG_LANES(2)
        BLDP_ARG_LANES(4)
        BLDP_ARG_LANES(8)
        BLDP_ARG_LANES(16)
        BLDP_ARG_LANES(32)
        BLDP_ARG_LANES(64)
      }
      break;
    case ARGEXT_BLOCK:
      hipLaunchKernelGGL((vec ? k_arg_block<true> : k_arg_block<false>), grid, dim3(kBlock), 0, s,
                         a);
      return hipGetLastError();
  }
#undef BLDP_ARG_LANES
  return hipErrorInvalidValue;
}

}  // namespace bldp
