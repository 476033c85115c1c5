// Internal launch interface shared by kernels.hip and api.hip (not part of the ABI).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "bldp.h"

namespace bldp {

// Record the thread-local error message returned by bldp_last_error; returns code.
int set_error(int code, const char *fmt, ...);

// Library-owned device scratch cached per (device, stream).  A lease keeps
// the (device, stream) entry locked until it is destroyed: take it before the
// first launch that uses the buffer and keep it until the last is queued, so
// host threads sharing a stream never interleave their kernels on it.
// Growing synchronizes that stream first.
struct ScratchLease {
  void *ptr = nullptr;
  std::unique_lock<std::mutex> hold;
};
int scratch_lease(hipStream_t s, size_t bytes, ScratchLease *lease);
// bldp_bslz4_decode_dev_async with chunk k's host header at comp_host +
// (chunk_off[k] - host_base) (bslz4.hip; the chunk reader's slot ring)
int bslz4_decode_async_at(int nchunk, const uint8_t *comp_host, uint64_t host_base,
                          const uint8_t *comp_dev, const uint64_t *chunk_off,
                          const uint64_t *chunk_len, int elem_size, uint8_t *out_dev,
                          const uint64_t *out_off, const uint64_t *out_len, int *err_dev,
                          hipStream_t s);
std::vector<int> scratch_devices();  // devices holding scratch
void scratch_release_all();          // frees it (callers drained the devices)
// The native file readers (fileio.hip): stop the reader threads and free the
// pinned slot ring (waits for a read call in progress).
void fileio_release();

// A host-staging pipeline (runtime.hip): two streams and four cached device
// buffers (slots 0/1 = input of stream 0/1, 2/3 = output of stream 0/1).
struct Stager {
  int dev = -1;
  hipStream_t st[2] = {nullptr, nullptr};
  void *buf[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t bytes[4] = {0, 0, 0, 0};
  std::vector<void *> temp;  // oversize buffers of the current call
};
// Take an idle pipeline of `dev` (created on first use); the device must be gfx950.
int stager_acquire(int dev, Stager **out);
// Device buffer of >= need bytes for `slot`, valid until stager_release.
int stager_buffer(Stager *s, int slot, size_t need, void **p);
void stager_release(Stager *s);
// The library's persistent worker stream on `dev`.
int device_stream(int dev, hipStream_t *out);

// One reduction launch: nbank banks with identical geometry.
// Window element (c, i, t) of bank b sits at
//   in[b][in_off + c*in_cs + i*in_ld_i + t*in_ld_t]
// and output element (c', i, t') of bank b is written at
//   out[b*out_bank + c' + i*out_ld_i + t'*out_ld_t].
struct RedArgs {
  const float *in[BLDP_MAX_BANKS];
  float *out;
  float *ws;  // partials [nchunk][nbank][nto][ni][nco] when nchunk > 1
  int64_t out_bank, out_ld_i, out_ld_t;
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t nco, ni, nto, F, T;
  int64_t rows_per_chunk;  // time rows of one T-block handled by one block
  int64_t blocks_c;        // blocks along the output-channel axis
  int64_t ntiles;          // workgroup tiles (grid may be smaller: grid-stride)
  int32_t nchunk, nbank;
  int32_t ts;              // waves of a tile that split the T rows (1, 2, 4)
  int32_t k4;              // float4 loads per lane per row (vector path)
  int32_t vec_out;         // narrow path: 16/8-byte output stores are legal
  int64_t gpt;             // tile path: output channels (groups) per workgroup tile
  int32_t tpb;             // row path: time blocks per workgroup (k_reduce_rowt when > 1)
  int32_t tsub_log2;       // k_reduce_rowt: log2 of the time groups sharing a workgroup
  int32_t bpack;           // k_reduce_rowt: the 2^tsub_log2 lane sets take consecutive banks;
                           // lane path: k_reduce_lanes (lanes along the stitched row)
  int32_t rsplit;          // k_reduce_rows: slices of a workgroup splitting a block's rows (1 = k_reduce_row)
  int32_t st_plain;        // row / il / rowt output stores plain (1) or non-temporal (0)
  int32_t xcd_lg;          // log2 XCDs of the per-XCD tile order (xcd_order), 0 = off
  float div;               // F*T, the mean divisor
  int32_t qrank;           // quantile: the lower rank j - 1 (0-based; the upper is qrank + 1 < F)
  double qg;               // quantile: the weight g of the upper rank
};

// Runtime plan options (bldp_plan_option): process-wide overrides of the
// planners' choices, for tests that enumerate every form of a plan and for
// A/B timing in one process.  plan_opt returns the override, or the option's
// default (the measured choice) when there is none; -1 = "the planner
// decides by shape" where an option has that setting (row_split).
// Names and defaults: kernels.hip kPlanOpts.
enum PlanOpt {
  OPT_ROW_SPLIT = 0, OPT_TS_FILL, OPT_NARROW_MIS, OPT_T38,
  OPT_WIDE_SPLIT, OPT_NARROW_TPB, OPT_LANE, OPT_LANE3, OPT_LANET, OPT_LANET_PACK, OPT_VEC_IL,
  OPT_VEC_ROW, OPT_ROW_TPB, OPT_ROWT_PACK, OPT_ROWT_SMALL, OPT_WAVET, OPT_UNALIGNED_VEC,
  OPT_KURT_EXACT, OPT_KURT_MID_CPL, OPT_KURT_MID_SMALL, OPT_KURT_LEAF_NARROW, OPT_KURT_LEAF_TILE,
  OPT_TYPED_VEC, OPT_TYPED_KURT, OPT_ROW_BPACK, OPT_LANE_BPACK, OPT_WAVE_BPACK, OPT_COL3, OPT_ROWT_NARROW8, OPT_ST_PLAIN, OPT_COUNT
};
int64_t plan_opt(int k);
inline int64_t opt(int k) { return plan_opt(k); }
// name -> option index, or -1
int plan_opt_index(const char *name);
int64_t plan_opt_override(int k);  // -1 = none
bool plan_opt_valid(int k, int64_t v);  // v in the option's domain (or < 0: the default)
void plan_opt_domain(int k, int64_t *lo, int64_t *hi);
void plan_opt_set(int k, int64_t v);

enum Path { PATH_VEC = 0, PATH_NARROW = 1, PATH_SCALAR = 2, PATH_TILE = 3, PATH_VEC_IL = 4,
            PATH_VEC_ROW = 5, PATH_NARROW_MIS = 6, PATH_LANE = 7,
            // median / var / std (stats.hip): the moments kernels, the bitonic
            // sort of blocks of <= 64, the radix select with the block's keys in
            // registers, and the radix select that re-reads the block every pass
            PATH_MOMENTS = 8, PATH_MEDIAN_SORT = 9, PATH_MEDIAN_SELECT = 10,
            PATH_MEDIAN_STREAM = 11 };

// The kernel a Float32 reduce plan starts: one value per k_reduce_* entry of
// kernels.hip (plan_reduce chooses, launch_reduce switches on it).
enum ReduceKernel { RK_VEC = 0, RK_WAVET, RK_IL, RK_ROW, RK_ROWS, RK_ROWT, RK_NARROW, RK_NARROWT,
                    RK_NARROW_MIS, RK_LANE, RK_LANET, RK_LANES, RK_COL3, RK_TILE, RK_SCALAR,
                    RK_COUNT };

struct Plan {
  int path;
  int lpg;                   // lanes per output group (vector path; stats.hip: 256 = a workgroup)
  int64_t grid;             // blocks of 256 threads
  int64_t nout;              // outputs per bank
  size_t ws_bytes;           // partial workspace required (0 if nchunk == 1)
  // plan_reduce only: the kernel and its launch, as launch_reduce starts them
  int kernel;                // ReduceKernel
  int nrw;                   // k_reduce_rowt / narrowt: rows per lane (their NRW)
  uint32_t gx, gy, gz;       // grid
  uint32_t block;            // threads per workgroup
  uint32_t shm;              // dynamic LDS bytes
};

// Choose the kernel and fill its launch (the plan's kernel and geometry, and
// ts, k4, nchunk, rows_per_chunk, blocks_c, ntiles, ... of the args, as that
// kernel reads them) for an args struct whose shape/stride fields are set.
// `aligned` says whether 16-byte vector loads of every group are legal;
// `rows16` whether every bank pointer is 16-byte aligned and the IF/time
// pitches are multiples of 4 floats (any channel offset and step); `words`
// whether the channel step is 1 and every bank pointer is dword-aligned.
// xcd_lg: log2 of the device's XCD count (0: one XCD, or not a power of two)
Plan plan_reduce(RedArgs &a, bool aligned, bool rows16, bool words, int num_cus, int xcd_lg);

hipError_t launch_reduce(const RedArgs &a, const Plan &p, int op, hipStream_t s);
// events the next launch_reduce's dispatches carry (null, null: none)
void set_launch_events(hipEvent_t start, hipEvent_t stop);
// those events, for the next dispatch (the start event is handed out once)
void take_launch_events(hipEvent_t *start, hipEvent_t *stop);
// One dispatch of kn; it carries the thread's timing events when they are set
// (hipExtLaunchKernel).  shm: dynamic LDS bytes; a workgroup's allocation above
// 64 KiB needs the kernel's attribute raised.
template <typename... Args>
hipError_t launch_kernel(void (*kn)(Args...), dim3 grid, dim3 block, unsigned shm, hipStream_t s,
                         Args... args) {
  if (shm > 65536u)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kn),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  take_launch_events(&ev_start, &ev_stop);
  if (ev_stop)
    hipExtLaunchKernelGGL(kn, grid, block, shm, s, ev_start, ev_stop, 0, args...);
  else
    hipLaunchKernelGGL(kn, grid, block, shm, s, args...);
  return hipGetLastError();
}

// Workgroup x of a launch of X in the per-XCD contiguous order over 2^lg
// XCDs: x runs on XCD x % 2^lg and takes tile (x % 2^lg) * (X / 2^lg) +
// x / 2^lg.  lg = 0 (the plan's "no"), or a grid 2^lg does not divide: x.
__device__ __forceinline__ uint32_t xcd_order(uint32_t x, uint32_t X, int lg) {
  const uint32_t m = (1u << lg) - 1u;
  if (lg == 0 || (X & m)) return x;
  return (x & m) * (X >> lg) + (x >> lg);
}

// median / var / std of the F channels of every block (stats.hip); T = 1.
// plan_stats fills the launch geometry like plan_reduce (`words`: the channel
// step is 1 and every bank pointer is dword-aligned) and returns BLDP_OK or,
// with the message recorded, BLDP_EINVAL for a launch too large for one grid.
// (op 7 is unassigned; BLDP_OP_MAD = 8 takes the median's kernels and plans)
inline bool stat_op(int op) {
  return (op >= BLDP_OP_VAR && op <= BLDP_OP_MEDIAN) || op == BLDP_OP_MAD;
}
// quantile(p) is no op of the ABI (its entry points carry p, not an op): inside
// the library it travels as kOpQuantile with the rank and weight in the args.
constexpr int kOpQuantile = 64;
// the ops that take the median's kernels and plans
// quantiles(ps), the bldp_quantiles_* entry points: several quantiles of every
// block from one selection; the ranks travel in a QSet beside the args.
constexpr int kOpQuantiles = 65;
inline bool median_op(int op) {
  return op == BLDP_OP_MEDIAN || op == BLDP_OP_MAD || op == kOpQuantile || op == kOpQuantiles;
}
// What the median's kernels select (their compile-time selector): ranks
// (n-1)/2 and n/2 once, the same twice (mad), or the run-time ranks qrank and
// qrank + 1 joined by quantile_of, or the ranks of a QSet joined plane by plane.
// SEL_OUTLIERS: mad's two selections, then the flags of an OutlArgs.
enum Sel { SEL_MEDIAN = 0, SEL_MAD = 1, SEL_QUANTILE = 2, SEL_QUANTILES = 3, SEL_OUTLIERS = 4 };
// The 0-based lower rank j - 1 and the weight g of Statistics.quantile(x, p)
// of n >= 2 values (type 7), in Float64 with every operation rounded once
// (host.hip); the upper rank is always *rank + 1 <= n - 1.
void quantile_rank(int64_t n, double p, int64_t *rank, double *g);
// mad: the median of |x - median(x)| times StatsBase's Float64 mad_constant
// (1 / quantile(Normal(), 3/4)), the product rounded once more to Float32
__device__ __forceinline__ float mad_scale(float m) {
  return (float)((double)m * 1.4826022185056018);
}
// |x - c|, the difference rounded once (never fused into a neighbour)
__device__ __forceinline__ float abs_dev(float x, float c) {
#pragma clang fp contract(off)
  return fabsf(__fsub_rn(x, c));
}
// Statistics' quantile from the keys' values a = v[j], b = v[j + 1] and the
// weight g: a + g * (b - a) with the difference rounded once to Float32 and
// the product and the sum once each in Float64 where both are finite, else
// (1 - g) * a + g * b (NaN for a zero weight next to an infinity: the formula
// as it stands); the result rounded to Float32.  Never fused: the products
// and sums are written as operators under the pragma, because hipcc contracts
// by default and __dmul_rn / __dadd_rn are ordinary operators of a header
// compiled without it (they came out as v_fmac_f64 here).
__device__ __forceinline__ float quantile_mix(float a, float b, double g) {
#pragma clang fp contract(off)
  double r;
  if (isfinite(a) && isfinite(b)) {
    const float d = b - a;
    const double gd = g * (double)d;
    r = (double)a + gd;
  } else {
    const double w = 1.0 - g;
    const double wa = w * (double)a, gb = g * (double)b;
    r = wa + gb;
  }
  return (float)r;
}
// The rank set of quantiles(ps) for blocks of n >= 2 values: a by-value kernel
// argument of the SEL_QUANTILES instantiations alone (RedArgs and TStatArgs,
// which every hot reduce kernel carries, stay as they are).  Plane k of the
// output is quantile_of(key of rank[lo[k]], key of rank[hi[k]], g[k]) and lies
// k * out_ld_q elements after plane 0.
struct QSet {
  int32_t np;                             // planes: 1 .. BLDP_MAX_QUANTILES
  int32_t nr;                             // distinct ranks
  int32_t nlow;                           // distinct lower ranks
  int32_t rank[2 * BLDP_MAX_QUANTILES];   // {j_k - 1, j_k} over all k: sorted, distinct, 0-based
  int32_t low[BLDP_MAX_QUANTILES];        // {j_k - 1} over all k: sorted, distinct
  uint8_t lo[BLDP_MAX_QUANTILES];         // plane k: where rank[] holds j_k - 1
  uint8_t hi[BLDP_MAX_QUANTILES];         // ... and j_k
  uint8_t lsel[BLDP_MAX_QUANTILES];       // ... and where low[] holds j_k - 1
  double g[BLDP_MAX_QUANTILES];           // plane k: the weight of the upper rank
  int64_t out_ld_q;                       // plane stride of the output (elements)
};
// Builds it with quantile_rank (host.hip); 1 <= np <= BLDP_MAX_QUANTILES, every
// p in [0, 1], n >= 2.
void quantile_set(int64_t n, int np, const double *p, int64_t out_ld_q, QSet *qs);
// outliers (the bldp_outliers_* entry points): what the SEL_OUTLIERS
// instantiations of the median's kernels write beside their args, a by-value
// kernel argument of those alone (as QSet).  med, mad and count are laid out as
// the args lay out `out` (which these launches leave null): element e of `out`
// is element e of each.  mask is the window's flags: element (c, i, t) of bank b
// at mask[b * mask_bank + c + i * mask_ld_i + t * mask_ld_t].  A null pointer is
// neither formed nor stored.
struct OutlArgs {
  double nsigma;  // finite, >= +0.0
  float *med, *mad;
  uint32_t *count;
  uint8_t *mask;
  int64_t mask_bank, mask_ld_i, mask_ld_t;
};
// The threshold of a block whose scaled mad is s: Float32(nsigma * Float64(s)),
// one product rounded once (NaN for a NaN s, and for 0 * Inf: nothing is flagged)
__device__ __forceinline__ float outl_thr(double nsigma, float s) {
  return (float)(nsigma * (double)s);
}
// four flags (0 / 1) at m .. m + 3: one dword where the address allows it
__device__ __forceinline__ void outl_store4(uint8_t *m, bool f0, bool f1, bool f2, bool f3) {
  if (((uintptr_t)m & 3u) == 0) {
    *reinterpret_cast<uint32_t *>(m) =
        (uint32_t)f0 | ((uint32_t)f1 << 8) | ((uint32_t)f2 << 16) | ((uint32_t)f3 << 24);
  } else {
    m[0] = f0, m[1] = f1, m[2] = f2, m[3] = f3;
  }
}
int plan_stats(RedArgs &a, int op, bool words, int xcd_lg, Plan *p);
hipError_t launch_stats(const RedArgs &a, const Plan &p, int op, hipStream_t s);
// kOpQuantiles: the median's plan (plan_stats) launched with the rank set
hipError_t launch_stats_q(const RedArgs &a, const Plan &p, const QSet &qs, hipStream_t s);
// reads of the block a quantiles launch of that plan makes (any rank set)
int stats_q_reads(const Plan &p);
// outliers: mad's plan (plan_stats with BLDP_OP_MAD) launched with the OutlArgs
hipError_t launch_stats_outl(const RedArgs &a, const Plan &p, const OutlArgs &oa, hipStream_t s);
// reads of the block an outliers launch of that plan makes
int stats_outl_reads(const Plan &p, bool mask);

// argmax / argmin of every F x T block (argext.hip): the offset k + F * tt of the
// winner in its block (column-major, channel fastest), first occurrence, NaN
// first of all; optionally the winner's bits.  r is the reduce's geometry
// (r.out: the value output or null; r.ts / r.tsub_log2: the time slices of a
// workgroup that split a block's rows; r.k4: float4 loads per lane per row, 0 =
// one dword per element).  plan_argext fills the launch geometry like plan_stats.
struct ArgArgs {
  RedArgs r;
  uint32_t *idx;  // output (c', i, t') of bank b at idx[b*out_bank + c' + i*out_ld_i + t'*out_ld_t]
  uint32_t inv;   // 0 = argmax, 0xffffffff = argmin (the key is inverted)
};
enum ArgExtPath { ARGEXT_LANES = 0, ARGEXT_LANES_TSPLIT = 1, ARGEXT_BLOCK = 2 };
int plan_argext(ArgArgs &a, bool words, int num_cus, int xcd_lg, Plan *p);
hipError_t launch_argext(const ArgArgs &a, const Plan &p, hipStream_t s);

// Masked reduce of every F x T block (masked.hip): the sum or mean of the
// samples whose flag is 0 and their count.  r is the reduce's geometry (r.out:
// the sum / mean output or null), filled by plan_argext: the walk is argext's.
// Flag (c, i, t) of bank b's selected window at
//   mask[b*m_bank + c*m_cs + i*m_ld_i + t*m_ld_t]  (bytes; a stride of 0 broadcasts).
// A by-value kernel argument of the masked kernels alone (RedArgs and ArgArgs
// stay as they are).
struct MaskedArgs {
  RedArgs r;
  uint32_t *kept;  // output (c', i, t') of bank b at kept[b*out_bank + c' + i*out_ld_i + t'*out_ld_t], or null
  const uint8_t *mask;
  int64_t m_cs, m_ld_i, m_ld_t, m_bank;
  int32_t mform;   // MaskForm (plan_masked)
  int32_t mean;    // 1: the sum divided once by Float32(kept)
};
// How the flags are loaded: a byte per element at the strided address, one
// aligned dword for the four flags of a float4, one byte per row (m_cs == 0).
enum MaskForm { MASK_BYTE = 0, MASK_DWORD = 1, MASK_ROW = 2 };
// The bytes that the mask of an (NC, ni, nt) window reaches from its pointer on,
// with the (non-negative) strides ld; a stride of 0 adds nothing.
inline size_t mask_span_bytes(int64_t NC, int64_t ni, int64_t nt, const int64_t ld[3]) {
  return (size_t)((NC - 1) * ld[0] + (ni - 1) * ld[1] + (nt - 1) * ld[2] + 1);
}
// plan_argext's plan (paths ArgExtPath) plus the mask form; `mask_words`: the
// mask pointer is 4-byte aligned.  Filled without a GPU.
int plan_masked(MaskedArgs &a, bool words, bool mask_words, int num_cus, int xcd_lg, Plan *p);
hipError_t launch_masked(const MaskedArgs &a, const Plan &p, hipStream_t s);

// Histogram of every F x T block (hist.hip): B bins of [lo, hi) and the below,
// above and nan counts, B + 3 planes of uint32.  Window element (c, i, t) of bank
// b at in[b][in_off + c*in_cs + i*in_ld_i + t*in_ld_t]; plane q of block
// (c', i, t') of bank b at out[b*out_bank + c' + i*out_ld_i + t'*out_ld_t +
// q*out_ld_q].  A by-value kernel argument of the histogram kernels alone.
struct HistArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  uint32_t *out;
  int64_t out_bank, out_ld_i, out_ld_t, out_ld_q;
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t nco, ni, nto, F, T;
  int32_t nbank;
  int32_t B;        // bins: 1 .. BLDP_MAX_HIST_BINS
  float lo, hi, s;  // Float32(lo), Float32(hi), Float32(B) / (hi - lo)
  // the plan (plan_hist)
  int32_t vec;     // float4 loads, else one dword per element
  int32_t G;       // blocks of a workgroup, neighbours along the channels
  int32_t R;       // replicas of a block's counters in LDS (a power of two)
  int32_t wlog2;   // log2 of a workgroup's lanes along the channels
  int32_t atomic;  // a block is shared by workgroups: atomicAdd into the zeroed out
  int32_t nchunk;  // chunks of a block's T rows
  int64_t rows_per_chunk;
  int64_t ctiles;      // G == 1: column tiles of a block's F channels
  int64_t tile_items;  // items (float4s or dwords) of a workgroup's row
  int64_t ncg;         // channel groups: ceil(nco / G), or nco * ctiles
};
enum HistPath { HIST_BLOCK = 0, HIST_BLOCK_SPLIT = 1, HIST_LANES = 2, HIST_LANES_TSPLIT = 3 };
// Fills the plan of an args struct whose shape, stride and B fields are set
// (`words`: the channel step is 1 and every bank pointer is dword-aligned), without
// a GPU.  p: path (HistPath), lpg = the lanes along the channels, grid = workgroups
// per bank, shm = LDS bytes.  BLDP_OK or, with the message recorded, BLDP_EINVAL for
// a launch too large for one grid.
int plan_hist(HistArgs &a, bool words, int num_cus, Plan *p);
// Zeroes the output first when a.atomic, on the same stream.
hipError_t launch_hist(const HistArgs &a, const Plan &p, hipStream_t s);

// The flagged samples of a window as an ordered list (hits.hip).  The window is
// the vcat (NC = nbank*nc, ni, nt) of the banks, N elements in the linear order
// k = c + NC*(i + ni*t); element k of bank b = c / nc at in[b][in_off + (c % nc)*in_cs
// + i*in_ld_i + t*in_ld_t], its flag at mask[c*m_cs + i*m_ld_i + t*m_ld_t] (bytes).
// idx[j] / val[j], j < min(total, cap): the j-th flagged k and that sample's bits;
// a null list is not written.  A by-value kernel argument of the hits kernels alone.
struct HitsArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  const uint8_t *mask;
  int64_t *idx;
  uint32_t *val;
  uint64_t *total;
  uint64_t *woff;    // workspace: the tiles' list offsets [tiles]
  uint32_t *wcount;  // workspace: the tiles' flag counts [tiles]
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t nc, NC, ni, nt, N;
  int64_t m_cs, m_ld_i, m_ld_t;
  int64_t cap;
  // the plan (plan_hits)
  int64_t E;       // elements of a tile, a multiple of 256 * W
  int64_t tiles;   // ceil(N / E), one workgroup each
  int32_t nbank;
  int32_t mform;   // MaskForm (MASK_DWORD: one aligned load of W flags)
  int32_t W;       // flags per lane per load: 1, 4 or 16
  int32_t mdense;  // the flag of element k is mask[k]
};
// The kernels of a plan: k_hits_count / k_hits_write over bytes, dwords of 4
// flags, 16-byte loads of 16 flags, or (the count alone) one byte per row.
enum HitsKernel { HITS_BYTE = 0, HITS_WIDE4 = 1, HITS_WIDE16 = 2, HITS_ROW = 3 };
// Fills the plan of an args struct whose shape, stride and mask fields are set,
// without a GPU; mask_addr: the mask pointer (its alignment chooses the load; 0
// counts as aligned).  p: path = the MaskForm, lpg = W, grid = gx = the tiles,
// nout = the chunks the scan loops over, ws_bytes, kernel = the HitsKernel.
// BLDP_OK or, with the message recorded, BLDP_EINVAL for more tiles than one
// launch takes.
int plan_hits(HitsArgs &a, uintptr_t mask_addr, Plan *p);
// count, scan and (write) the list kernel, on one stream
hipError_t launch_hits(const HitsArgs &a, const Plan &p, bool write, hipStream_t s);

// Fold of a window over its coarse channels (fold.hip): output (k, i, t') is the
// Float64 sum (or mean) of the unflagged samples A[k + nfpc*j, i, t'*T + tt] of
// every bank, rounded once to Float32, and their count.  Window element (c, i, t)
// of bank b at in[b][in_off + c*in_cs + i*in_ld_i + t*in_ld_t], its flag at
// mask[b*m_bank + c*m_cs + i*m_ld_i + t*m_ld_t] (bytes), output (k, i, t') at
// [k + i*out_ld_i + t'*out_ld_t] of out and kept (a null one is not written).
// A by-value kernel argument of the fold kernels alone.
struct FoldArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  float *out;
  uint32_t *kept;
  const uint8_t *mask;
  double *ws_sum;     // workspace (nchunk > 1): the chunks' sums [nchunk][nto][ni][nfpc]
  uint32_t *ws_kept;  // ... and their counts, behind the sums
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t m_cs, m_ld_i, m_ld_t, m_bank;
  int64_t out_ld_i, out_ld_t;
  int64_t nfpc, J, ni, T, nto;
  int32_t nbank;
  int32_t mean;          // 1: the sum divided once in Float64 by Float64(kept)
  int32_t mask_present;  // 0: everything is kept, no flag is loaded
  // the plan (plan_fold)
  int32_t vec;     // float4 loads, else one dword per element
  int32_t mform;   // MaskForm, or FOLD_MASK_NONE
  int32_t rows;    // FoldPath
  int32_t nchunk;  // chunks of a block's units, a workgroup each
  int32_t mew;     // the merge: outputs of a workgroup (a power of two <= 64)
  int64_t P;       // items (float4s or values) of a coarse channel
  int64_t G;       // coarse channels a workgroup's lanes cover (cols: 1)
  int64_t xwg;     // cols: workgroups along k
  int64_t JG;      // ceil(J / G)
  int64_t U, CU;   // units (bank, coarse group, spectrum) of a block; units per chunk
  int64_t nout;    // nfpc * ni * nto
};
enum FoldPath { FOLD_COLS = 0, FOLD_ROWS = 1 };
constexpr int FOLD_MASK_NONE = 3;  // beside MaskForm's 0 .. 2
// Fills the plan of an args struct whose shape, stride and mask fields are set,
// without a GPU (`vec`: 16-byte loads of every item are legal when nfpc % 4 == 0;
// `mask_words`: the mask pointer is 4-byte aligned).  p: path (FoldPath), lpg = the
// lanes along the channels, grid = the fold's workgroups, nout, ws_bytes.  BLDP_OK
// or, with the message recorded, BLDP_EINVAL for a launch too large for one grid.
int plan_fold(FoldArgs &a, bool vec, bool mask_words, int num_cus, Plan *p);
// the fold and, when a.nchunk > 1, the merge, on one stream
hipError_t launch_fold(const FoldArgs &a, const Plan &p, hipStream_t s);

// Unfold (fold.hip): out[b*nc + c + i*out_ld_i + t*out_ld_t] = A_b[c, i, t] / or -
// prof[c mod nfpc + i*prof_ld_i + (t div T)*prof_ld_t], one rounded Float32
// operation.  A by-value kernel argument of k_unfold alone.
struct UnfoldArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  const float *prof;
  float *out;
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t prof_ld_i, prof_ld_t, out_ld_i, out_ld_t;
  int64_t nc, ni, nt, nfpc, T;
  int32_t nbank;
  int32_t sub;  // 0 divide, 1 subtract
  int32_t vec;  // float4 loads and stores (plan_unfold)
};
// Sets a.vec (`vec`: 16-byte accesses of the window, the profile and the output are
// legal when nfpc % 4 == 0) and returns the workgroups per bank.
int64_t plan_unfold(UnfoldArgs &a, bool vec);
hipError_t launch_unfold(const UnfoldArgs &a, int64_t grid, hipStream_t s);

// Drift-rate sums of every channel (dedoppler.hip): S[c, i, b, d] = the Float32 sum
// over t = 0 .. T-1, in that order, of A[c + off(d, t), i, b*T + t] inside the
// segment of c, for d = -D .. D; best / drift: the greatest sum and its d over the
// scan 0, -1, +1, ..., -D, +D (bldp.h has the rule).  Window element (c, i, t) of
// bank k at in[k][in_off + c*in_cs + i*in_ld_i + t*in_ld_t]; output (c, i, b) of
// bank k at [k*out_bank + c + i*out_ld_i + b*out_ld_t] of best and drift, drift d's
// plane of sums at + (d + D)*out_ld_q (a null output is not written).  A by-value
// kernel argument of k_dedoppler alone.
struct DedopArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  float *best;
  int32_t *drift;
  float *sums;
  int64_t out_bank, out_ld_i, out_ld_t, out_ld_q;
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t nc, ni, nb, T;
  int64_t seg;  // channels of a segment; 0: the whole window
  int32_t nbank;
  int32_t D;
  // the plan (plan_dedoppler)
  int32_t vec;  // rows staged by float4 loads, else a dword at a time
  int32_t C;    // channels of a tile = lanes of a workgroup
  int32_t H;    // halo channels staged on each side (>= D)
  int32_t RW;   // words of a staged row: C + 2H
  int32_t R;    // rows of a staging chunk (resident: T)
  int64_t tiles;
};
enum DedopPath { DEDOP_RESIDENT = 0, DEDOP_CHUNKED = 1 };
enum DedopKernel { DEDOP_K_VEC = 0, DEDOP_K_SCALAR = 1 };
// Fills the plan of an args struct whose shape, stride, seg and D fields are set,
// without a GPU (`vec`: 16-byte loads of every aligned float4 of the rows are
// legal).  p: path (DedopPath), lpg = block = C, grid = workgroups per bank, gx / gy
// / gz, shm = LDS bytes, kernel (DedopKernel), nrw = the drift groups, nout,
// ws_bytes = 0.  BLDP_OK or, with the message recorded, BLDP_EINVAL for a launch too
// large for one grid.
int plan_dedoppler(DedopArgs &a, bool vec, Plan *p);
int dedoppler_group();  // drifts of a group
hipError_t launch_dedoppler(const DedopArgs &a, const Plan &p, hipStream_t s);

// median / var / std of every block of T selected spectra of every (channel,
// IF) column (tstats.hip): tavfunc, fqav's rule on the time axis.  Window
// element (c, i, t) of bank k at in[k][in_off + c*in_cs + i*in_ld_i +
// t*in_ld_t], output (c, i, b) at out[k*out_bank + c + i*out_ld_i + b*out_ld_b].
struct TStatArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  float *out;
  int32_t nbank;
  int32_t vec;      // float4 columns (4 channels per lane), else one
  int32_t lx_log2;  // split form: log2 of a workgroup's lanes along the channels
  int32_t xcd_lg;   // log2 XCDs of the per-XCD tile order, 0 = off
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t nc, ni, T, nb;
  int64_t ncg;      // column groups: nc / (4 or 1)
  int64_t ctiles;   // split form: channel tiles of 2^lx_log2 column groups
  int64_t out_bank, out_ld_i, out_ld_b;
  // chunked moments: a block's spectra in nchunk chunks of tchunk, one workgroup
  // each; ws holds the partials, Float64 [2][nchunk][nbank][nb][ni][nc]
  int32_t nchunk;
  int64_t tchunk;
  double *ws;
  int32_t qrank;  // quantile: the lower rank j - 1 (0-based; the upper is qrank + 1 < T)
  double qg;      // quantile: the weight g of the upper rank
};
enum TStatPath { TSTAT_REGS_MOMENTS = 0, TSTAT_REGS_MEDIAN = 1, TSTAT_SPLIT_MOMENTS = 2,
                 TSTAT_SPLIT_MEDIAN = 3, TSTAT_CHUNK_MOMENTS = 4 };
struct TStatPlan {
  int path;
  int cpl;          // channels per lane
  int tsplit;       // time slices of a workgroup splitting a block (1: register form)
  int passes;       // reads of the block
  int64_t grid;     // workgroups of 256 threads (per bank)
  size_t ws_bytes;  // workspace (the chunked moments' partials, else 0)
};
// Fills the launch geometry of an args struct whose shape / stride fields are
// set (`words`: every bank pointer is dword-aligned); BLDP_OK or, with the
// message recorded, BLDP_EINVAL for a launch too large for one grid.
int plan_tstat(TStatArgs &a, int op, bool words, int num_cus, int xcd_lg, TStatPlan *p);
hipError_t launch_tstat(const TStatArgs &a, const TStatPlan &p, int op, hipStream_t s);
// kOpQuantiles: plan_tstat's median plan, its split form re-tiled for nlow
// distinct lower ranks (tstats.hip: ranks per sweep, columns per workgroup,
// p->passes = the reads of the block), and its launch with the rank set
int plan_tstat_q(TStatArgs &a, int nlow, bool words, int num_cus, int xcd_lg, TStatPlan *p);
hipError_t launch_tstat_q(const TStatArgs &a, const TStatPlan &p, const QSet &qs, hipStream_t s);
// outliers: mad's plan (plan_tstat with BLDP_OP_MAD) launched with the OutlArgs,
// and the reads of the block that launch makes
hipError_t launch_tstat_outl(const TStatArgs &a, const TStatPlan &p, const OutlArgs &oa,
                             hipStream_t s);
int tstat_outl_reads(const TStatPlan &p, bool mask);

hipError_t launch_stitch(int nbank, const float *g, int64_t nc, int64_t nrows, float *out,
                         hipStream_t s);
hipError_t launch_despike(float *d, int64_t nchan, int64_t nrows, int64_t nfpc, int64_t nspike,
                          hipStream_t s);

// Kurtosis launch (kurtosis.hip).  Julia's Float32 mean is a pairwise sum
// whose halving tree is perfect down to level K ("blocks", <= 2048 spectra),
// each block being one or two sequentially summed leaves (<= 1024 spectra).
struct KurtArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  int32_t nbank;
  int64_t nrow;                     // nbank * ni output rows of nc channels
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t nc, ni, nt;
  int32_t vec;  // float4 along channels legal
  int32_t rows16;  // ... and every float4 is 16-byte aligned (global_load_lds)
  int32_t K;    // level of the blocks of the pairwise-sum tree
  int64_t nslot;  // leaf slots, 2 per block (2^(K+1))
  int64_t nseg;   // 64-lane column segments per row (k_kurt_leaf)
  int32_t leafw;  // channels per lane of k_kurt_leaf (kLeafW; 1 for short narrow windows)
  int32_t leaftile;  // leaves read whole into registers: k_kurt_tile's lane groups per channel (0 = streamed)
  // two-pass (unaligned) z pass
  int64_t rows_per_chunk;
  int32_t nchunk;
  int32_t ts;       // waves of a workgroup splitting the spectra of a tile (1, 2, 4)
  float *mean;      // [nbank*ni][nc]  Float32 mean (two-pass path)
  double *ws_mom;   // [nchunk][2][nbank*ni][nc] (order kOrdAll: [nchunk][3])
  // leaf / tree-node partials: pm [4][nodes][n] Float64 (mean, M2, M3, M4
  // about the node's own mean), pf [3][nodes][n] Float32 (pairwise sum, max, min)
  double *pm;
  float *pf;
  double *out;      // [nbank][ni][nc]
  int32_t order;    // the moment: 4 = kurtosis, 3 = skewness, kOrdAll = every plane
                    // of `mo` (set before plan_kurtosis)
  // order kOrdAll (getmoments): the planes mean, var = cm2/n, skewness and
  // kurtosis, each [nbank][ni][nc]; a null plane is neither formed nor stored
  double *mo[4];
};
// The third moment order: one pass keeps cm2, cm3 and cm4 and writes KurtArgs.mo
// (KurtBlkArgs.mo) instead of `out`.
constexpr int kOrdAll = 0;
enum { MO_MEAN = 0, MO_VAR = 1, MO_SKEW = 2, MO_KURT = 3 };
void plan_kurtosis(KurtArgs &k, int num_cus);
size_t kurtosis_ws_bytes(const KurtArgs &k);
hipError_t launch_kurtosis(KurtArgs &k, char *ws, hipStream_t s);
// Which kurtosis path a plan takes (0 registers, 1 register tile, 2 streamed
// leaves + tree merge, 3 two passes), for tests and bench.
int kurtosis_path(const KurtArgs &k);
int64_t kurtosis_max_grid(const KurtArgs &k);  // largest grid of the plan

// Kurtosis over blocks of M spectra, the one-launch form (kurtosis.hip):
// float4-column windows (unit channel step), M <= 1024.  Block b holds the
// window's spectra [b*M, (b+1)*M); output (c, i, b) of bank k at
// out[k*out_bank + c + i*out_ld_i + b*out_ld_b].
struct KurtBlkArgs {
  const float *in[BLDP_MAX_BANKS];  // banks with identical geometry
  int32_t nbank;
  int32_t leafw;  // channels per lane of the streamed form (M > 32)
  int64_t in_off, in_ld_i, in_ld_t;
  int64_t nc, ni, M, nb;
  int64_t out_bank, out_ld_i, out_ld_b;
  double *out;
  int32_t order;  // 4 = kurtosis, 3 = skewness, kOrdAll = the planes of `mo`
  double *mo[4];  // order kOrdAll: mean, var, skewness, kurtosis, each laid out as `out`
};
// `whole`: the KurtArgs of the whole window (its float4 columns are every block's)
bool kurt_blocks_fused(const KurtArgs &whole, int64_t M);
void plan_kurt_blocks(KurtBlkArgs &k, int num_cus);
int64_t kurt_blocks_grid(const KurtBlkArgs &k);
hipError_t launch_kurt_blocks(const KurtBlkArgs &k, hipStream_t s);
// block-by-block form: dense [nbank][ni][nc] results of one block into the product
hipError_t launch_kurt_scatter(const double *src, int64_t nbank, int64_t ni, int64_t nc,
                               double *out, int64_t out_bank, int64_t out_ld_i, hipStream_t s);

// Window of a chunked dataset: chunk dims (ct, ci, cc) in C order, a chunk
// bounding box starting at (bt0, bi0, bc0) with (gt, gi, gc) chunks, and the
// window {c0, nc, cs, i0, ni, is, t0, nt, ts} in dataset coordinates.
struct UnchunkArgs {
  int64_t ct, ci, cc, bt0, bi0, bc0, gt, gi, gc;
  int64_t c0, nc, cs, i0, ni, is, t0, nt, ts;
};
hipError_t launch_unchunk(const float *packed, const UnchunkArgs &u, float *out, hipStream_t s);

// Reductions and kurtosis of non-Float32 elements (typed.hip).  Element
// (c, i, t) of bank b at in[b][in_off + c*in_cs + i*in_ld_i + t*in_ld_t],
// output (c', i, t') at out[b*out_bank + c' + i*out_ld_i + t'*out_ld_t]
// (kurtosis: out dense [nbank][ni][nco], nto = the spectra).
struct TypedArgs {
  const void *in[BLDP_MAX_BANKS];
  void *out;
  int32_t dtype, nbank;
  int64_t out_bank, out_ld_i, out_ld_t;
  int64_t in_off, in_cs, in_ld_i, in_ld_t;
  int64_t nco, ni, nto, F, T;
  int32_t num_cus;  // of the launch's device (the coalesced kernel's grid)
  void *ws;         // typed kurtosis: kurtosis_typed_ws_bytes of scratch (or null)
  size_t ws_bytes;  // its size (the launch re-plans and checks it: plan options are
                    // process-wide, so another thread may change them in between)
};
size_t dtype_size(int dtype);              // 0 = unknown
int typed_out_dtype(int dtype, int op);    // -1 = invalid
hipError_t launch_reduce_typed(const TypedArgs &a, int op, hipStream_t s);
hipError_t launch_kurtosis_typed(const TypedArgs &a, double *out, hipStream_t s);
size_t kurtosis_typed_ws_bytes(const TypedArgs &a);  // scratch launch_kurtosis_typed wants

hipError_t launch_synth(float *out, int64_t nchan, int64_t nif, int64_t ntime, int64_t nfpc,
                        uint64_t seed, int kind, hipStream_t s);

}  // namespace bldp
