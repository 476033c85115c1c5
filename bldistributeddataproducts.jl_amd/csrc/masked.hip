// masked.hip — masked reduce of Float32 windows (gfx950): the sum (or mean) of
// the unflagged samples of every F x T block of the reduce, and how many there
// were, from one read of the window and one read of a byte mask.
//
// The block of output (c', i, t') is the reduce's: F selected channels by T
// selected spectra.  The mask is addressed in window coordinates: flag (c, i, t)
// of the selected window is mask[c*m_cs + i*m_ld_i + t*m_ld_t]; a stride of 0
// broadcasts.  A sample is kept when its byte is 0.  kept is the count of kept
// samples, sum their Float32 sum in any order, mean that sum divided once by
// Float32(kept).  A flagged sample is excluded by a select before the add, never
// multiplied: a flagged NaN or Inf leaves the result finite.
//
// The walk is argext.hip's (the plan is plan_argext's), with (sum, kept) in
// place of (key, off) and a second, byte-wide stream:
//   k_msk_lanes  (F <= 1024)  the 1 .. 64 lanes of a wave that share a block
//                stream its T rows, <= 16 elements a lane a row (float4 loads on
//                unit-step windows with F % 4 == 0, else one dword per element);
//                a lane with one item a row takes 4 (dwords: 16) rows a batch
//                where the rows are not split, else a row at a time.
//                The flags of a batch are loaded with its data, both behind the
//                previous batch's adds.  With ts > 1 time slices a workgroup
//                holds kBlock / (lanes * ts) blocks; the slices meet through LDS.
//   k_msk_block  (F > 1024)   one workgroup per block, rows streamed; the waves
//                meet once through LDS.
// The mask stream has three forms (MF): 0 a byte load per element at the strided
// address, 1 one aligned dword for a float4's four flags, 2 one byte per row
// (m_cs == 0: the flag is uniform over a row's channels).
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// Block g of bank blockIdx.y: its first element, its first flag and its output
// index; false past the end.
__device__ __forceinline__ bool msk_group(const MaskedArgs &a, int64_t g, const float *&p,
                                          const uint8_t *&m, int64_t &o) {
  const RedArgs &r = a.r;
  if (g >= r.nco * r.ni * r.nto) return false;
  int64_t co, q, i, t;
  divmod(g, r.nco, q, co);
  divmod(q, r.ni, t, i);
  const int64_t b = blockIdx.y;
  p = r.in[b] + r.in_off + co * r.F * r.in_cs + i * r.in_ld_i + t * r.T * r.in_ld_t;
  m = a.mask + b * a.m_bank + co * r.F * a.m_cs + i * a.m_ld_i + t * r.T * a.m_ld_t;
  o = b * r.out_bank + co + i * r.out_ld_i + t * r.out_ld_t;
  return true;
}

// The four flags of a float4 as one word, flag c in byte c.
template <int MF>
__device__ __forceinline__ uint32_t flags4(const uint8_t *e, int64_t cs) {
  if (MF == 1) return *reinterpret_cast<const uint32_t *>(e);
  return (uint32_t)e[0] | ((uint32_t)e[cs] << 8) | ((uint32_t)e[2 * cs] << 16) |
         ((uint32_t)e[3 * cs] << 24);
}

// One sample into the pair: the flag selects what is added.
__device__ __forceinline__ void msk_take(float &sum, uint32_t &kept, float x, bool flagged) {
  sum += flagged ? 0.0f : x;
  kept += flagged ? 0u : 1u;
}

// Store the block's result: the sum or the mean, and the count, where asked.
__device__ __forceinline__ void msk_store(const MaskedArgs &a, int64_t o, float sum,
                                          uint32_t kept) {
  if (a.r.out) a.r.out[o] = a.mean ? __fdiv_rn(sum, (float)kept) : sum;
  if (a.kept) a.kept[o] = kept;
}

// MR: a lane has one item (a float4 or a value) of a row, and its register
// slots hold that item of NS successive rows of its slice instead of NS items
// of one row (argext.hip k_arg_lanes).
template <int LPG, bool VEC, bool MR, int MF>
__global__ __launch_bounds__(kBlock) void k_msk_lanes(const MaskedArgs a) {
  __shared__ float shs[kBlock];  // the slices' pairs (ts > 1)
  __shared__ uint32_t shk[kBlock];
  const RedArgs &r = a.r;
  constexpr int GW = kBlock / LPG;          // lane groups of a workgroup: blocks x slices
  // register slots of a lane: 64 lanes take up to 16 values a lane a row, and a
  // batch is 4 (dwords: 16) rows; fewer than 64 lanes never hold more than one
  // item a lane (the plan takes the least power of two that covers a row)
  constexpr int NS = (!MR && LPG < 64) ? 1 : VEC ? 4 : 16;
  constexpr int EP = VEC ? 4 : 1;           // elements of a slot
  const int tl = r.tsub_log2;               // log2 of the time slices, 2^tl <= GW
  const int TS = 1 << tl, G = GW >> tl;     // time slices; blocks of a workgroup
  const int lg = threadIdx.x % LPG;
  const int gi = (threadIdx.x / LPG) & (G - 1);
  const uint32_t sl = (threadIdx.x / LPG) >> (__builtin_ctz(GW) - tl);
  const int64_t tile = xcd_order(blockIdx.x, gridDim.x, r.xcd_lg);
  const float *p = nullptr;
  const uint8_t *m = nullptr;
  int64_t o = 0;
  const bool ok = msk_group(a, tile * G + gi, p, m, o);
  const int F = (int)r.F;
  const uint32_t T = ok ? (uint32_t)r.T : 0u;
  const int64_t mcs = a.m_cs;
  // slot s of the batch that starts at row tt: item it(s) of row row(s, tt)
  auto it = [&](int s) { return MR ? lg : lg + s * LPG; };
  auto row = [&](int s, uint32_t tt) { return MR ? tt + (uint32_t)(s * TS) : tt; };
  auto has = [&](int s, uint32_t tt) { return EP * it(s) < F && (!MR || row(s, tt) < T); };
  // the data of a batch and its flags: f[s] holds slot s's (VEC: four, a byte
  // each); the row-uniform form keeps a row's one flag (not MR: in f[0])
  auto load = [&](float *d, uint32_t *f, uint32_t tt) {
    if (MF == 2 && !MR) f[0] = m[(int64_t)tt * a.m_ld_t];
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (has(s, tt)) {
        const float *q = p + (int64_t)row(s, tt) * r.in_ld_t;
        const uint8_t *mq = m + (int64_t)row(s, tt) * a.m_ld_t;
        if (VEC) {
          const float4 x = ld4(q + 4 * it(s));
          d[4 * s] = x.x, d[4 * s + 1] = x.y, d[4 * s + 2] = x.z, d[4 * s + 3] = x.w;
          if (MF != 2) f[s] = flags4<MF>(mq + 4 * it(s) * mcs, mcs);
        } else {
          d[s] = q[(int64_t)it(s) * r.in_cs];
          if (MF != 2) f[s] = mq[(int64_t)it(s) * mcs];
        }
        if (MF == 2 && MR) f[s] = mq[0];
      }
  };
  const uint32_t step = MR ? NS * TS : TS;  // rows between a slice's batches
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t kept = 0;
  float v[NS * EP] = {}, nx[NS * EP] = {};
  uint32_t f[NS] = {}, nf[NS] = {};
  if (sl < T) load(v, f, sl);
#pragma unroll 2
  for (uint32_t tt = sl; tt < T; tt += step) {
    if (tt + step < T) load(nx, nf, tt + step);  // in flight under this batch's adds
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (has(s, tt)) {
#pragma unroll
        for (int c = 0; c < EP; ++c) {
          const uint32_t w = MF == 2 ? (MR ? f[s] : f[0]) : VEC ? (f[s] >> (8 * c)) & 0xffu : f[s];
          msk_take(acc[(VEC ? c : s) & 3], kept, v[EP * s + c], w != 0u);
        }
      }
#pragma unroll
    for (int u = 0; u < NS * EP; ++u) v[u] = nx[u];
#pragma unroll
    for (int u = 0; u < NS; ++u) f[u] = nf[u];
  }
  float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int w = LPG / 2; w >= 1; w /= 2) {
    sum += __shfl_xor(sum, w, 64);
    kept += __shfl_xor(kept, w, 64);
  }
  if (TS > 1) {  // (uniform)
    if (lg == 0) shs[gi + G * sl] = sum, shk[gi + G * sl] = kept;
    __syncthreads();
    if (sl == 0 && lg == 0)
      for (int s = 1; s < TS; ++s) sum += shs[gi + G * s], kept += shk[gi + G * s];
  }
  if (ok && sl == 0 && lg == 0) msk_store(a, o, sum, kept);
}

template <bool VEC, int MF>
__global__ __launch_bounds__(kBlock) void k_msk_block(const MaskedArgs a) {
  __shared__ float shs[kBlock / 64];
  __shared__ uint32_t shk[kBlock / 64];
  const RedArgs &r = a.r;
  const uint32_t tid = threadIdx.x;
  const float *p = nullptr;
  const uint8_t *m = nullptr;
  int64_t o = 0;
  if (!msk_group(a, blockIdx.x, p, m, o)) return;  // (uniform)
  const uint32_t F = (uint32_t)r.F, T = (uint32_t)r.T;
  const uint32_t n = VEC ? F / 4 : F;  // items of a row: float4s or values
  const int64_t mcs = a.m_cs;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t kept = 0;
  for (uint32_t tt = 0; tt < T; ++tt) {
    const float *q = p + (int64_t)tt * r.in_ld_t;
    const uint8_t *mq = m + (int64_t)tt * a.m_ld_t;
    const uint32_t rf = MF == 2 ? mq[0] : 0u;  // the row's one flag
#pragma unroll 4
    for (uint32_t k = tid; k < n; k += kBlock) {
      if (VEC) {
        const float4 x = ld4(q + 4 * (int64_t)k);
        const uint32_t w = MF == 2 ? 0u : flags4<MF>(mq + 4 * (int64_t)k * mcs, mcs);
        msk_take(acc[0], kept, x.x, MF == 2 ? rf != 0u : (w & 0xffu) != 0u);
        msk_take(acc[1], kept, x.y, MF == 2 ? rf != 0u : (w & 0xff00u) != 0u);
        msk_take(acc[2], kept, x.z, MF == 2 ? rf != 0u : (w & 0xff0000u) != 0u);
        msk_take(acc[3], kept, x.w, MF == 2 ? rf != 0u : (w & 0xff000000u) != 0u);
      } else {
        const uint32_t w = MF == 2 ? rf : mq[(int64_t)k * mcs];
        msk_take(acc[0], kept, q[(int64_t)k * r.in_cs], w != 0u);
      }
    }
  }
  float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int w = 32; w >= 1; w /= 2) {
    sum += __shfl_xor(sum, w, 64);
    kept += __shfl_xor(kept, w, 64);
  }
  if ((tid & 63) == 0) shs[tid >> 6] = sum, shk[tid >> 6] = kept;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) sum += shs[w], kept += shk[w];
    msk_store(a, o, sum, kept);
  }
}

// the lanes kernel of a plan's form
template <int LPG>
void (*msk_lanes_kernel(bool vec, bool mr, int mf))(const MaskedArgs) {
  switch ((vec ? 1 : 0) | (mr ? 2 : 0) | (mf << 2)) {
    case 0: return k_msk_lanes<LPG, false, false, 0>;
    case 1: return k_msk_lanes<LPG, true, false, 0>;
    case 2: return k_msk_lanes<LPG, false, true, 0>;
    case 3: return k_msk_lanes<LPG, true, true, 0>;
    case 5: return k_msk_lanes<LPG, true, false, 1>;
    case 7: return k_msk_lanes<LPG, true, true, 1>;
    case 8: return k_msk_lanes<LPG, false, false, 2>;
    case 9: return k_msk_lanes<LPG, true, false, 2>;
    case 10: return k_msk_lanes<LPG, false, true, 2>;
    case 11: return k_msk_lanes<LPG, true, true, 2>;
  }
  return nullptr;  // (dword flags go with float4 data only)
}

}  // namespace

int plan_masked(MaskedArgs &ma, bool words, bool mask_words, int num_cus, int xcd_lg, Plan *pp) {
  // the walk and its launch geometry are argext's
  ArgArgs aa{};
  aa.r = ma.r;
  const int rc = plan_argext(aa, words, num_cus, xcd_lg, pp);
  if (rc)
    return set_error(rc, "masked reduce: %lld blocks of %lld x %lld are too many for one launch",
                     (long long)(ma.r.nco * ma.r.ni * ma.r.nto), (long long)ma.r.F,
                     (long long)ma.r.T);
  ma.r = aa.r;
  const RedArgs &a = ma.r;
  // A float4's flags as one dword: unit channel stride and every flag address
  // that is formed a multiple of 4 (F % 4 == 0 makes every item's offset one).
  const bool pitch4 = (a.ni <= 1 || ma.m_ld_i % 4 == 0) &&
                      (a.nto * a.T <= 1 || ma.m_ld_t % 4 == 0) &&
                      (a.nbank <= 1 || ma.m_bank % 4 == 0);
  if (ma.m_cs == 0)
    ma.mform = MASK_ROW;
  else if (a.k4 != 0 && ma.m_cs == 1 && mask_words && pitch4)
    ma.mform = MASK_DWORD;
  else
    ma.mform = MASK_BYTE;
  return BLDP_OK;
}

hipError_t launch_masked(const MaskedArgs &a, const Plan &p, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  const dim3 grid((unsigned)p.grid, (unsigned)a.r.nbank);
  const bool vec = a.r.k4 != 0;
  const int mf = a.mform;
  if (mf < MASK_BYTE || mf > MASK_ROW || (mf == MASK_DWORD && !vec)) return hipErrorInvalidValue;
  // a lane with one item a row batches rows where the rows are not split
  // (launch_argext's rule and measurements)
  const int64_t items = vec ? a.r.F / 4 : a.r.F;
  const bool mr = a.r.ts == 1 && a.r.T > 1 && items <= p.lpg;
  if (p.path != ARGEXT_BLOCK && p.lpg < 64 && items > p.lpg) return hipErrorInvalidValue;
  void (*kn)(const MaskedArgs) = nullptr;
  switch (p.path) {
    case ARGEXT_LANES:
    case ARGEXT_LANES_TSPLIT:
      switch (p.lpg) {
        case 1: kn = msk_lanes_kernel<1>(vec, mr, mf); break;
        case 2: kn = msk_lanes_kernel<2>(vec, mr, mf); break;
        case 4: kn = msk_lanes_kernel<4>(vec, mr, mf); break;
        case 8: kn = msk_lanes_kernel<8>(vec, mr, mf); break;
        case 16: kn = msk_lanes_kernel<16>(vec, mr, mf); break;
        case 32: kn = msk_lanes_kernel<32>(vec, mr, mf); break;
        case 64: kn = msk_lanes_kernel<64>(vec, mr, mf); break;
      }
      break;
    case ARGEXT_BLOCK:
      kn = vec ? (mf == MASK_DWORD  ? k_msk_block<true, 1>
                  : mf == MASK_ROW ? k_msk_block<true, 2>
                                   : k_msk_block<true, 0>)
               : (mf == MASK_ROW ? k_msk_block<false, 2> : k_msk_block<false, 0>);
      break;
  }
  if (!kn) return hipErrorInvalidValue;
  return launch_kernel(kn, grid, dim3(kBlock), 0, s, a);
}

}  // namespace bldp
