// hits.hip — the flagged samples of a Float32 window as an ordered list (gfx950):
// Julia's findall(!iszero, mask) and A[mask] on the device.
//
// The window's linear order k = c + NC*(i + ni*t) (column-major, NC = nbank*nc
// channels of the vcat window) is cut into tiles of E elements, a contiguous run
// of k each, one workgroup per tile.  Three launches on one stream:
//   k_hits_count  reads only the mask and leaves every tile's flag count
//                 (uint32) in the workspace;
//   k_hits_scan   one workgroup: the exclusive prefix of the tile counts as
//                 uint64 offsets, in chunks of kScanChunk tiles with a carry,
//                 and the total;
//   k_hits_write  a tile with no flags, or whose offset is >= cap, leaves after
//                 its two workspace words (uniform).  Else it reads its flags
//                 again and ranks every flagged sample in k order: inside a
//                 wave by ballot and mbcnt (one flag a lane) or by a prefix of
//                 the lanes' popcounts (4 or 16 flags a lane), across the waves
//                 through LDS, across the tile's steps by a running base.  Only
//                 flagged samples are loaded from the window.
// A lane owns W consecutive k of a step, a wave 64*W, a step 256*W: the position
// in the list is a function of k alone.  Integer adds only; no atomics, no
// workgroup waits on another.
// The mask stream has three forms (MF, masked.hip's): 0 a byte per element at
// the strided address, 1 one aligned load of W = 4 or 16 flags (unit channel
// stride, NC % W == 0, pointer and pitches multiples of W), 2 one byte per row
// (m_cs == 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bldp_impl.h"

namespace bldp {
namespace {

constexpr int kBlock = 256;                       // 4 waves of 64
constexpr int kScanPer = 8;                       // tiles of a lane of the scan
constexpr int kScanChunk = kBlock * kScanPer;     // tiles of one pass of the scan
constexpr int kMinSteps = 4;                      // steps of the smallest tile
constexpr int64_t kMaxTiles = 8192;               // of one call
constexpr int64_t kMaxTileElems = (int64_t)1 << 31;  // a tile's count is uint32

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

// byte offset of window element k's flag
__device__ __forceinline__ int64_t mask_off(const HitsArgs &a, int64_t k) {
  if (a.mdense) return k;  // (uniform)
  int64_t q, c, t, i;
  divmod(k, a.NC, q, c);
  divmod(q, a.ni, t, i);
  return c * a.m_cs + i * a.m_ld_i + t * a.m_ld_t;
}

// bit c of the result: byte c of x is not 0
__device__ __forceinline__ uint32_t nz4(uint32_t x) {
  const uint32_t h = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
  return (h | (h >> 7) | (h >> 14) | (h >> 21)) & 0xfu;
}

// The flags of elements k .. k + W - 1 (all inside the window and, W > 1, inside
// one row): bit j is element k + j's.
template <int W>
__device__ __forceinline__ uint32_t flags(const HitsArgs &a, int64_t k) {
  const uint8_t *m = a.mask + mask_off(a, k);
  if (W == 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(m);
    return nz4(v.x) | (nz4(v.y) << 4) | (nz4(v.z) << 8) | (nz4(v.w) << 12);
  }
  if (W == 4) return nz4(*reinterpret_cast<const uint32_t *>(m));
  return *m != 0 ? 1u : 0u;
}

// the tile of workgroup x: elements [k0, k1)
__device__ __forceinline__ void tile_run(const HitsArgs &a, int64_t x, int64_t &k0, int64_t &k1) {
  k0 = x * a.E;
  k1 = k0 + a.E < a.N ? k0 + a.E : a.N;
}

template <int MF, int W>
__global__ __launch_bounds__(kBlock) void k_hits_count(const HitsArgs a) {
  __shared__ uint32_t sh[kBlock / 64];
  const uint32_t tid = threadIdx.x;
  int64_t k0, k1;
  tile_run(a, blockIdx.x, k0, k1);
  uint32_t n = 0;
  if (MF == 2) {
    // a row's one byte counts for the part of the row inside the tile
    int64_t r0, r1, c;
    divmod(k0, a.NC, r0, c);
    divmod(k1 - 1, a.NC, r1, c);
    for (int64_t r = r0 + tid; r <= r1; r += kBlock) {
      int64_t t, i;
      divmod(r, a.ni, t, i);
      const uint32_t f = a.mask[i * a.m_ld_i + t * a.m_ld_t];
      const int64_t lo = r * a.NC > k0 ? r * a.NC : k0;
      const int64_t hi = (r + 1) * a.NC < k1 ? (r + 1) * a.NC : k1;
      n += f != 0u ? (uint32_t)(hi - lo) : 0u;
    }
  } else {
#pragma unroll 4
    for (int64_t k = k0 + (int64_t)tid * W; k < k1; k += kBlock * W)
      n += (uint32_t)__popc(flags<W>(a, k));
  }
#pragma unroll
  for (int w = 32; w >= 1; w /= 2) n += __shfl_xor(n, w, 64);
  if ((tid & 63) == 0) sh[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) n += sh[w];
    a.wcount[blockIdx.x] = n;
  }
}

__global__ __launch_bounds__(kBlock) void k_hits_scan(const HitsArgs a) {
  __shared__ uint64_t sh[kBlock / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t carry = 0;  // flags of the chunks before this one (uniform)
  for (int64_t c0 = 0; c0 < a.tiles; c0 += kScanChunk) {  // (uniform)
    const int64_t j0 = c0 + (int64_t)tid * kScanPer;
    uint32_t c[kScanPer];
    uint64_t s = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
      c[u] = j0 + u < a.tiles ? a.wcount[j0 + u] : 0u;
      s += c[u];
    }
    uint64_t inc = s;  // the inclusive prefix over the wave's lanes
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
      const uint64_t v = __shfl_up((unsigned long long)inc, d, 64);
      if (lane >= (uint32_t)d) inc += v;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
      const uint64_t v = sh[w];
      before += w < wave ? v : 0;
      all += v;
    }
    __syncthreads();  // (sh is written again by the next chunk)
    uint64_t o = carry + before + (inc - s);
#pragma unroll
    for (int u = 0; u < kScanPer; ++u)
      if (j0 + u < a.tiles) {
        a.woff[j0 + u] = o;
        o += c[u];
      }
    carry += all;
  }
  if (tid == 0) *a.total = carry;
}

template <int W>
__global__ __launch_bounds__(kBlock) void k_hits_write(const HitsArgs a) {
  __shared__ uint32_t sh[2][kBlock / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t cnt = a.wcount[blockIdx.x];
  const uint64_t first = a.woff[blockIdx.x], cap = (uint64_t)a.cap;
  if (cnt == 0u || first >= cap) return;  // (uniform)
  int64_t k0, k1;
  tile_run(a, blockIdx.x, k0, k1);
  uint64_t base = first;  // list position of the step's first flag (uniform)
  int par = 0;
  uint32_t fnext = k0 + (int64_t)tid * W < k1 ? flags<W>(a, k0 + (int64_t)tid * W) : 0u;
  for (int64_t s = k0; s < k1; s += kBlock * W, par ^= 1) {  // (uniform)
    const int64_t k = s + (int64_t)tid * W;
    const uint32_t f = fnext;
    // the next step's flags, in flight under this step's ranks and gathers
    fnext = k + kBlock * W < k1 ? flags<W>(a, k + kBlock * W) : 0u;
    uint32_t ex, wt;  // flags of the wave's lanes below this one; of the wave
    if (W == 1) {
      const uint64_t b = __ballot(f != 0u);
      ex = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
      wt = (uint32_t)__popcll(b);
    } else {
      const uint32_t n = (uint32_t)__popc(f);
      uint32_t inc = n;
#pragma unroll
      for (int d = 1; d < 64; d *= 2) {
        const uint32_t v = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += v;
      }
      ex = inc - n;
      wt = __shfl(inc, 63, 64);
    }
    // sh[par] is next written two steps on, behind the next step's barrier
    if (lane == 0) sh[par][wave] = wt;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
      const uint32_t v = sh[par][w];
      before += w < wave ? v : 0u;
      all += v;
    }
    uint64_t r = base + before + ex;
    for (uint32_t g = f; g != 0u && r < cap; g &= g - 1u, ++r) {
      const int64_t kk = k + (__ffs(g) - 1);
      // the sample, through the reduce's geometry
      int64_t q, cc, t, i, b = 0, c;
      divmod(kk, a.NC, q, cc);
      divmod(q, a.ni, t, i);
      c = cc;
      if (a.nbank > 1) divmod(cc, a.nc, b, c);
      const float *p = a.in[b] + a.in_off + c * a.in_cs + i * a.in_ld_i + t * a.in_ld_t;
      if (a.idx) a.idx[r] = kk;
      if (a.val) a.val[r] = *reinterpret_cast<const uint32_t *>(p);
    }
    base += all;
    if (base >= cap || base - first >= cnt) break;  // (uniform) nothing left to list
  }
}

}  // namespace

int plan_hits(HitsArgs &a, uintptr_t mask_addr, Plan *p) {
  const auto pitch = [&](int64_t w) {
    return a.NC % w == 0 && mask_addr % (uintptr_t)w == 0 && (a.ni <= 1 || a.m_ld_i % w == 0) &&
           (a.nt <= 1 || a.m_ld_t % w == 0);
  };
  if (a.m_cs == 0)
    a.mform = MASK_ROW, a.W = 1;
  else if (a.m_cs == 1 && pitch(16))
    a.mform = MASK_DWORD, a.W = 16;
  else if (a.m_cs == 1 && pitch(4))
    a.mform = MASK_DWORD, a.W = 4;
  else
    a.mform = MASK_BYTE, a.W = 1;
  a.mdense = a.m_cs == 1 && (a.ni <= 1 || a.m_ld_i == a.NC) &&
             (a.nt <= 1 || a.m_ld_t == a.NC * a.ni);
  // the smallest tile is kMinSteps steps; it doubles until kMaxTiles cover the window
  a.E = (int64_t)kMinSteps * kBlock * a.W;
  while ((a.N + a.E - 1) / a.E > kMaxTiles && a.E < kMaxTileElems) a.E *= 2;
  a.tiles = (a.N + a.E - 1) / a.E;
  if (a.tiles > kMaxTiles)
    return set_error(BLDP_EINVAL, "hits: %lld tiles of %lld elements are too many for one launch "
                     "(at most %lld)", (long long)a.tiles, (long long)a.E, (long long)kMaxTiles);
  p->path = a.mform;
  p->lpg = a.W;
  p->grid = a.tiles;
  p->nout = (a.tiles + kScanChunk - 1) / kScanChunk;  // passes of the scan
  p->ws_bytes = (size_t)a.tiles * (sizeof(uint64_t) + sizeof(uint32_t));
  p->kernel = a.mform == MASK_DWORD ? (a.W == 16 ? HITS_WIDE16 : HITS_WIDE4)
              : a.mform == MASK_ROW ? HITS_ROW
                                    : HITS_BYTE;
  p->gx = (uint32_t)a.tiles, p->gy = p->gz = 1;
  p->block = kBlock;
  p->shm = 0;
  return BLDP_OK;
}

hipError_t launch_hits(const HitsArgs &a, const Plan &p, bool write, hipStream_t s) {
  if (p.grid <= 0) return hipSuccess;
  if (!a.wcount || !a.woff || !a.total || !a.mask) return hipErrorInvalidValue;
  const dim3 grid(p.gx), block(p.block);
  void (*kc)(const HitsArgs) = nullptr, (*kw)(const HitsArgs) = nullptr;
  switch (p.kernel) {
    case HITS_BYTE: kc = k_hits_count<0, 1>, kw = k_hits_write<1>; break;
    case HITS_WIDE4: kc = k_hits_count<1, 4>, kw = k_hits_write<4>; break;
    case HITS_WIDE16: kc = k_hits_count<1, 16>, kw = k_hits_write<16>; break;
    case HITS_ROW: kc = k_hits_count<2, 1>, kw = k_hits_write<1>; break;
  }
  if (!kc) return hipErrorInvalidValue;
  hipError_t e = launch_kernel(kc, grid, block, 0, s, a);
  if (e != hipSuccess) return e;
  e = launch_kernel(k_hits_scan, dim3(1), block, 0, s, a);
  if (e != hipSuccess || !write) return e;
  return launch_kernel(kw, grid, block, 0, s, a);
}

}  // namespace bldp
