// hist.hip — histogram of Float32 windows (gfx950): for every F x T block of the
// reduce, how many samples fall into each of B equal bins of [lo, hi), how many
// lie below, above, and how many are NaN, from one streaming read of the window.
//
// The rule (include/bldp.h "Histogram"): a sample x goes, in this order, to
// `nan` when x != x, to `below` when x < lo, to `above` when x >= hi, else to bin
// min(floor((x - lo) * s), B - 1) with s = Float32(B) / (hi - lo) formed on the
// host.  The subtraction and the product are two Float32 operations, each rounded
// once (__fsub_rn, __fmul_rn: nothing to contract).  A sample is classed before
// it is converted to an integer, and the index is clamped before it addresses
// anything.  Counts are integers: the result does not depend on how lanes, waves
// and workgroups share a block.
//
// One kernel, k_hist, walks a rectangle of the window: rows [r0, r1) of a time
// block by a span of channels, W = 2^wlog2 lanes along the channels (float4 loads
// on unit-step windows, else one dword per element) and 256 / W rows at a time.
// It counts into LDS with ds_add_u32 and flushes once.  The plan (plan_hist)
// shapes the rectangle:
//   G == 1  the span is a block's F channels, or one of `ctiles` column tiles of
//           them, and the block's T rows go in `nchunk` chunks: a block is one
//           workgroup ("block": plain stores) or ctiles * nchunk of them
//           ("block_split": merged by atomicAdd into the zeroed output).
//   G > 1   the span is G blocks that are neighbours along the channels, one
//           item a lane a row, so that blocks of few channels still load whole
//           rows; every block has its own counters ("lanes"), and long blocks are
//           chunked over workgroups as above ("lanes_tsplit").
// LDS holds (B + 3) x S counters, S = G * R slots, as h[plane * S + slot]: a
// lane's slot is its block's g * R plus a replica lane % R, so that the lanes of
// a wave which hit one hot bin add to different words, and to different banks
// (plane-major: neighbouring slots are neighbouring dwords).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bldp_impl.h"

namespace bldp {
namespace {

constexpr int kBlock = 256;  // 4 waves of 64
// a float4 on any dword boundary (kernels.hip f4u)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

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

// The plane of a sample: 0 .. B-1 a bin, B below, B + 1 above, B + 2 nan.
__device__ __forceinline__ uint32_t hist_plane(float x, float lo, float hi, float s, uint32_t B) {
#pragma clang fp contract(off)
  const float d = __fsub_rn(x, lo);
  const float m = __fmul_rn(d, s);
  // classed first: only lo <= x < hi is converted (0 <= m, m <= about B)
  const bool in = x >= lo && x < hi;
  const uint32_t k = (uint32_t)(in ? m : 0.0f);  // m >= 0: truncation is floor
  uint32_t q = min(k, B - 1u);
  q = x < lo ? B : q;
  q = x >= hi ? B + 1u : q;
  q = x != x ? B + 2u : q;
  return q;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_hist(const HistArgs a) {
  extern __shared__ uint32_t h[];  // [B + 3][S]
  constexpr int EP = VEC ? 4 : 1;  // elements of an item
  const uint32_t tid = threadIdx.x;
  const uint32_t B = (uint32_t)a.B, NP = B + 3u;
  const uint32_t G = (uint32_t)a.G, R = (uint32_t)a.R, S = G * R;
  for (uint32_t k = tid; k < NP * S; k += kBlock) h[k] = 0u;
  // the rectangle of this workgroup: channel group cgi of IF i, chunk ch of time block to
  int64_t x1, x2, cgi, i, ch, to;
  divmod((int64_t)blockIdx.x, a.ncg, x1, cgi);
  divmod(x1, a.ni, x2, i);
  divmod(x2, a.nchunk, to, ch);
  int64_t co0, k0, k1;  // first block; the items [k0, k1) of a row, counted from co0's first channel
  uint32_t ng = 1;      // blocks of this workgroup
  if (G > 1) {
    co0 = cgi * G;
    ng = (uint32_t)min((int64_t)G, a.nco - co0);
    k0 = 0;
    k1 = (int64_t)ng * a.F / EP;
  } else {
    int64_t ct;
    divmod(cgi, a.ctiles, co0, ct);
    k0 = ct * a.tile_items;
    k1 = min(a.F / EP, k0 + a.tile_items);
  }
  const int64_t r0 = ch * a.rows_per_chunk, r1 = min(a.T, r0 + a.rows_per_chunk);
  const float *p = a.in[blockIdx.y] + a.in_off + co0 * a.F * a.in_cs + i * a.in_ld_i +
                   to * a.T * a.in_ld_t;
  const uint32_t W = 1u << a.wlog2, RP = kBlock >> a.wlog2;
  const uint32_t lx = tid & (W - 1u), ry = tid >> a.wlog2;
  // the slot of each element of this lane's item (G > 1: a lane has one item a row)
  uint32_t slot[EP];
#pragma unroll
  for (int e = 0; e < EP; ++e)
    slot[e] = G > 1 ? ((uint32_t)(EP * lx + e) / (uint32_t)a.F) * R + (lx & (R - 1u))
                    : (tid & (R - 1u));
  const float lo = a.lo, hi = a.hi, s = a.s;
  auto item = [&](int64_t r, int64_t k, float *v) {
    const float *q = p + r * a.in_ld_t;
    if (VEC) {
      const float4 f = ld4(q + 4 * k);
      v[0] = f.x, v[VEC ? 1 : 0] = f.y, v[VEC ? 2 : 0] = f.z, v[VEC ? 3 : 0] = f.w;
    } else {
      v[0] = q[k * a.in_cs];
    }
  };
  auto count = [&](const float *v) {
#pragma unroll
    for (int e = 0; e < EP; ++e) atomicAdd(&h[hist_plane(v[e], lo, hi, s, B) * S + slot[e]], 1u);
  };
  __syncthreads();
  constexpr int NB = 4;  // loads in flight per lane
  float v[NB][EP];
  if (k1 - k0 <= (int64_t)W) {  // (uniform) one item a lane a row: batches of rows
    const int64_t k = k0 + lx;
    if (k < k1)
      for (int64_t r = r0 + ry; r < r1; r += (int64_t)NB * RP) {
#pragma unroll
        for (int n = 0; n < NB; ++n)
          if (r + (int64_t)n * RP < r1) item(r + (int64_t)n * RP, k, v[n]);
#pragma unroll
        for (int n = 0; n < NB; ++n)
          if (r + (int64_t)n * RP < r1) count(v[n]);
      }
  } else {  // batches of items of a row
    for (int64_t r = r0 + ry; r < r1; r += RP)
      for (int64_t k = k0 + lx; k < k1; k += (int64_t)NB * W) {
#pragma unroll
        for (int n = 0; n < NB; ++n)
          if (k + (int64_t)n * W < k1) item(r, k + (int64_t)n * W, v[n]);
#pragma unroll
        for (int n = 0; n < NB; ++n)
          if (k + (int64_t)n * W < k1) count(v[n]);
      }
  }
  __syncthreads();
  // flush, in two steps.  First the R replicas of every counter meet: every lane
  // reads one word, neighbours neighbouring words (no bank is asked twice), the
  // replicas sit in R neighbouring lanes and are summed by xor-shuffles, and the
  // sum goes back to LDS as hc[plane * G + g].  Word idx / R is written only
  // after every word up to idx has been read (the barrier), and lies below every
  // word read later.
  if (R > 1u)
    for (uint32_t base = 0; base < NP * S; base += kBlock) {  // (uniform: S is a multiple of R)
      const uint32_t idx = base + tid;
      uint32_t c = idx < NP * S ? h[idx] : 0u;
      for (uint32_t w = R >> 1; w >= 1u; w >>= 1) c += __shfl_xor(c, (int)w, 64);
      __syncthreads();
      if (idx < NP * S && (idx & (R - 1u)) == 0u) h[idx / R] = c;
    }
  __syncthreads();
  // Then the counts leave, block g fastest: a plane's counts of neighbouring
  // blocks, or a lone block's neighbouring planes, go out in one instruction.
  uint32_t *o = a.out + (int64_t)blockIdx.y * a.out_bank + co0 + i * a.out_ld_i + to * a.out_ld_t;
  for (uint32_t idx = tid; idx < NP * ng; idx += kBlock) {
    const uint32_t q = idx / ng, g = idx - q * ng;
    const uint32_t c = h[q * G + g];
    uint32_t *d = o + g + (int64_t)q * a.out_ld_q;
    if (a.atomic) {
      if (c) atomicAdd(d, c);
    } else {
      *d = c;
    }
  }
}

// Zero the (nbank, nco, ni, nto, B + 3) counts that the split forms add into.
__global__ __launch_bounds__(kBlock) void k_hist_zero(const HistArgs a) {
  const int64_t NP = (int64_t)a.B + 3;
  const int64_t n = a.nco * a.ni * a.nto * NP * a.nbank;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * kBlock) {
    int64_t x1, x2, x3, co, i, to, q, b;
    divmod(e, a.nco, x1, co);
    divmod(x1, a.ni, x2, i);
    divmod(x2, a.nto, x3, to);
    divmod(x3, NP, b, q);
    a.out[b * a.out_bank + co + i * a.out_ld_i + to * a.out_ld_t + q * a.out_ld_q] = 0u;
  }
}

int64_t p2floor(int64_t v) {
  int64_t p = 1;
  while (2 * p <= v) p *= 2;
  return p;
}
int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// LDS words of a workgroup's counters: 48 KiB, so that three workgroups share a CU
constexpr int64_t kLdsWords = 12288;
// the fewest samples a workgroup of a split block takes, beside 4 per counter
// it flushes: below that the flush and the merge outweigh the count
constexpr int64_t kMinSamples = 32768;

}  // namespace

int plan_hist(HistArgs &a, bool words, int num_cus, Plan *pp) {
  const int64_t NP = (int64_t)a.B + 3, F = a.F, T = a.T;
  const int64_t gmax = kLdsWords / NP;  // blocks (times replicas) whose counters fit: >= 2
  // G > 1: neighbouring blocks of few channels share a workgroup's rows, at most
  // one item a lane (256 float4s or dwords) and as many as LDS holds
  int64_t G = 1;
  bool vec = false;
  if (a.nco > 1 && F <= 512) {
    const int64_t gv = p2floor(std::min(gmax, 1024 / F));
    const int64_t gs = F <= 128 ? p2floor(std::min(gmax, 256 / F)) : 1;
    if (words && (a.nco * F) % 4 == 0 && gv >= 2 && (gv * F) % 4 == 0)
      G = gv, vec = true;
    else if (gs >= 2)
      G = gs;
    while (G >= 2 && G / 2 >= a.nco) G /= 2;
    if (G == 1) vec = false;
  }
  if (G == 1) vec = words && F % 4 == 0;
  const int64_t EP = vec ? 4 : 1;
  const int64_t items = G * F / EP;  // of a workgroup's row, before column tiles
  const int64_t ncg0 = G > 1 ? ceil_div(a.nco, G) : a.nco;
  const int64_t n0 = ncg0 * a.ni * a.nto * a.nbank;
  // chunks of a block (a group of G): enough workgroups for four a CU, each with
  // kMinSamples samples and 4 a counter
  const int64_t target = 4 * (int64_t)std::max(num_cus, 1);
  const int64_t least = std::max(kMinSamples, 4 * NP * G);
  const int64_t want = std::max<int64_t>(
      1, n0 >= target ? 1 : std::min(G * F * T / least, ceil_div(target, std::max<int64_t>(n0, 1))));
  int64_t nchunk = std::min(want, T), ctiles = 1;
  if (G == 1) ctiles = std::max<int64_t>(1, std::min(ceil_div(want, nchunk), items / 256));
  const int64_t tile_items = ceil_div(items, ctiles);
  ctiles = ceil_div(items, std::max<int64_t>(tile_items, 1));
  int wlog2 = 0;
  while ((1 << wlog2) < 256 && (1 << wlog2) < tile_items) ++wlog2;
  const int64_t RP = 256 >> wlog2;
  int64_t rpc = ceil_div(T, nchunk);
  rpc = ceil_div(rpc, RP) * RP;
  nchunk = ceil_div(T, rpc);
  // replicas: the lanes of a half wave that share a block (G > 1), or 32, as LDS
  // allows; no more than a workgroup's samples can use (2 a counter)
  int64_t R = G > 1 ? std::min<int64_t>(std::max<int64_t>(1, F / EP), gmax / G) : gmax;
  R = std::min<int64_t>(R, std::max<int64_t>(1, tile_items * EP * rpc / (2 * NP * G)));
  R = p2floor(std::max<int64_t>(1, std::min<int64_t>(32, R)));
  a.vec = vec;
  a.G = (int32_t)G;
  a.R = (int32_t)R;
  a.wlog2 = wlog2;
  a.nchunk = (int32_t)nchunk;
  a.rows_per_chunk = rpc;
  a.ctiles = ctiles;
  a.tile_items = tile_items;
  a.ncg = G > 1 ? ncg0 : a.nco * ctiles;
  a.atomic = nchunk * ctiles > 1;
  const int64_t grid = a.ncg * a.ni * a.nto * nchunk;
  if (grid > INT32_MAX)
    return set_error(BLDP_EINVAL, "histogram: %lld blocks of %lld x %lld are too many for one "
                     "launch", (long long)(a.nco * a.ni * a.nto), (long long)F, (long long)T);
  *pp = Plan{};
  pp->path = G > 1 ? (nchunk > 1 ? HIST_LANES_TSPLIT : HIST_LANES)
                   : (a.atomic ? HIST_BLOCK_SPLIT : HIST_BLOCK);
  pp->lpg = 1 << wlog2;
  pp->grid = grid;
  pp->nout = a.nco * a.ni * a.nto;
  pp->ws_bytes = 0;
  pp->block = kBlock;
  pp->shm = (uint32_t)(NP * G * R * 4);
  return BLDP_OK;
}

hipError_t launch_hist(const HistArgs &a, const Plan &p, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  if (p.shm > 4 * kLdsWords || a.G < 1 || a.R < 1 || (a.R & (a.R - 1)) || a.wlog2 < 0 ||
      a.wlog2 > 8)
    return hipErrorInvalidValue;
  // G > 1: a lane has one item of the workgroup's row (its slots are per lane)
  if (a.G > 1 && (a.ctiles != 1 || a.tile_items > (1 << a.wlog2))) return hipErrorInvalidValue;
  if (a.atomic) {
    const int64_t n = a.nco * a.ni * a.nto * ((int64_t)a.B + 3) * a.nbank;
    const unsigned zg = (unsigned)std::min<int64_t>(ceil_div(n, kBlock), 16384);
    const hipError_t e = launch_kernel(k_hist_zero, dim3(zg), dim3(kBlock), 0, s, a);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)p.grid, (unsigned)a.nbank);
  return launch_kernel(a.vec ? k_hist<true> : k_hist<false>, grid, dim3(kBlock), p.shm, s, a);
}

}  // namespace bldp
