// api.hip — the extern "C" boundary of libbldp_hip (declared in include/bldp.h).
//
// Argument validation mirrors the reference's error behaviour:
//   * fqavby must divide the selected channel count (Julia reshape in
//     fqav, src/gbtworkerfunctions.jl:18-19 -> DimensionMismatch) => BLDP_EDIM;
//     the same rule is applied to tavby on the time axis;
//   * a window outside the array (h5["data"][idxs...] / dmmap[idxs...],
//     :174,:185 -> BoundsError) => BLDP_EBOUNDS;
//   * everything else that Julia would reject by type or @assert => BLDP_EINVAL.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "bldp_impl.h"

using namespace bldp;

namespace {

thread_local std::string g_err;

}  // namespace

int bldp::set_error(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {

#define fail bldp::set_error

#define HIPCHK(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) return fail(BLDP_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

// Resolved window: element (c, i, t) at base[off + c*cs + i*ld_i + t*ld_t].
struct Geo {
  int64_t nc, ni, nt;
  int64_t off, cs, ld_i, ld_t;
};

int resolve_window(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, Geo *g) {
  if (nchan < 0 || nif < 0 || ntime < 0)
    return fail(BLDP_EINVAL, "negative array dimension (%lld, %lld, %lld)", (long long)nchan,
                (long long)nif, (long long)ntime);
  const int64_t dims[3] = {nchan, nif, ntime};
  int64_t start[3], count[3], step[3];
  for (int ax = 0; ax < 3; ++ax) {
    if (win) {
      start[ax] = win[3 * ax];
      count[ax] = win[3 * ax + 1];
      step[ax] = win[3 * ax + 2];
    } else {
      start[ax] = 0;
      count[ax] = dims[ax];
      step[ax] = 1;
    }
    if (count[ax] < 0) return fail(BLDP_EINVAL, "negative window count on axis %d", ax + 1);
    if (count[ax] > 0) {
      if (step[ax] == 0) return fail(BLDP_EINVAL, "zero window step on axis %d", ax + 1);
      const int64_t last = start[ax] + (count[ax] - 1) * step[ax];
      if (start[ax] < 0 || start[ax] >= dims[ax] || last < 0 || last >= dims[ax])
        return fail(BLDP_EBOUNDS,
                    "BoundsError: window %lld:%lld:%lld (1-based) outside axis %d of size %lld",
                    (long long)(start[ax] + 1), (long long)step[ax], (long long)(last + 1),
                    ax + 1, (long long)dims[ax]);
    }
  }
  g->nc = count[0];
  g->ni = count[1];
  g->nt = count[2];
  const bool empty = g->nc == 0 || g->ni == 0 || g->nt == 0;
  g->off = empty ? 0 : start[0] + nchan * (start[1] + nif * start[2]);
  g->cs = step[0];
  g->ld_i = nchan * step[1];
  g->ld_t = nchan * nif * step[2];
  return BLDP_OK;
}

int resolve_factors(const Geo &g, int64_t fqavby, int64_t tavby, int64_t *F, int64_t *T) {
  *F = fqavby <= 1 ? 1 : fqavby;  // fqav: n <= 1 returns A (src/gbtworkerfunctions.jl:17)
  *T = tavby <= 1 ? 1 : tavby;
  if (g.nc % *F != 0)
    return fail(BLDP_EDIM, "DimensionMismatch: fqavby=%lld does not divide nchan=%lld",
                (long long)*F, (long long)g.nc);
  if (g.nt % *T != 0)
    return fail(BLDP_EDIM, "DimensionMismatch: tavby=%lld does not divide ntime=%lld",
                (long long)*T, (long long)g.nt);
  return BLDP_OK;
}

// ---- the front end the block operations share --------------------------------
// An operation's prepare is its own checks and fields, its planner call and a
// list of these; `what` is the prefix of the family's messages ("" the reduce's).
int check_nbank(int nbank) {
  if (nbank < 1 || nbank > BLDP_MAX_BANKS)
    return fail(BLDP_EINVAL, "nbank=%d outside 1..%d", nbank, BLDP_MAX_BANKS);
  return BLDP_OK;
}

// The window and the factors of its blocks.
int resolve_blocks(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int64_t fqavby,
                   int64_t tavby, Geo *g, int64_t *F, int64_t *T) {
  const int rc = resolve_window(nchan, nif, ntime, win, g);
  return rc ? rc : resolve_factors(*g, fqavby, tavby, F, T);
}

// counts, sums and offsets within a block are 31-bit (Python and the shim read
// Int32).  F <= nc and T <= nt: the product cannot overflow int64 for arrays
// that exist, and is checked by division anyway.
int check_block31(const char *what, int64_t F, int64_t T) {
  if (F > INT32_MAX / T)
    return fail(BLDP_EINVAL, "%sblocks of fqavby x tavby = %lld x %lld elements are beyond "
                "2^31 - 1", what, (long long)F, (long long)T);
  return BLDP_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

// The banks and the window's strides of any args struct; *words / *rows16: every
// bank pointer is 4 / 16-byte aligned (a null one counts as aligned).
template <class A>
int set_window(const char *what, A &a, const Geo &g, int nbank, const float *const *in,
               bool *words = nullptr, bool *rows16 = nullptr) {
  if (!in) return fail(BLDP_EINVAL, "%snull input pointer array", what);
  a.nbank = nbank;
  a.in_off = g.off, a.in_cs = g.cs, a.in_ld_i = g.ld_i, a.in_ld_t = g.ld_t;
  bool w = true, r = true;
  for (int b = 0; b < nbank; ++b) {
    a.in[b] = in[b];
    w = w && aligned4(in[b]);
    r = r && aligned16(in[b]);
  }
  if (words) *words = w;
  if (rows16) *rows16 = r;
  return BLDP_OK;
}

int check_banks(const char *what, int nbank, const float *const *in) {
  for (int b = 0; b < nbank; ++b)
    if (!in[b]) return fail(BLDP_EINVAL, "%snull input pointer (bank %d)", what, b);
  return BLDP_OK;
}

// The F x T blocks of a window and where their results go: output (c', i, t') of
// bank b at [b*out_bank + c' + i*out_ld_i + t'*out_ld_t].  True when there is none.
template <class A>
bool set_blocks(A &a, const Geo &g, int64_t F, int64_t T, int64_t out_bank, int64_t out_ld_i,
                int64_t out_ld_t) {
  a.nco = g.nc / F, a.ni = g.ni, a.nto = g.nt / T, a.F = F, a.T = T;
  a.out_bank = out_bank, a.out_ld_i = out_ld_i, a.out_ld_t = out_ld_t;
  return a.nco == 0 || a.ni == 0 || a.nto == 0;
}

// The dense vcat of nbank (d[0], d[1], d[2]) products: bank k's channels at k*d[0]
// of every (IF, time) row.
void vcat_layout(int nbank, const int64_t d[3], int64_t *bank, int64_t *ld_i, int64_t *ld_t) {
  *bank = d[0];
  *ld_i = nbank * d[0];
  *ld_t = nbank * d[0] * d[1];
}

// What a band entry point checks before its run, and where its dense product
// goes: l = {out_bank, out_ld_i, out_ld_t, out_ld_q} of the vcat of the banks.
int band_layout(int nbank, int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                int64_t fqavby, int64_t tavby, int64_t l[4]) {
  int rc = check_nbank(nbank);
  if (rc) return rc;
  Geo g;
  int64_t F, T;
  rc = resolve_blocks(nchan, nif, ntime, win, fqavby, tavby, &g, &F, &T);
  if (rc) return rc;
  const int64_t d[3] = {g.nc / F, g.ni, g.nt / T};
  vcat_layout(nbank, d, &l[0], &l[1], &l[2]);
  l[3] = l[2] * d[2];
  return BLDP_OK;
}

int check_out_strides(const char *what, int nbank, int64_t out_bank, int64_t ld_i, int64_t ld_t,
                      int64_t d0, int64_t d1, int64_t d2) {
  if (ld_i < d0 || ld_t < (d1 - 1) * ld_i + d0 || (nbank > 1 && out_bank < d0))
    return fail(BLDP_EINVAL, "%sout strides (%lld, %lld) overlap for a (%lld, %lld, %lld) result",
                what, (long long)ld_i, (long long)ld_t, (long long)d0, (long long)d1,
                (long long)d2);
  return BLDP_OK;
}

// The strides of a mask of an (NC, ni, .) window: the dense ones, or the caller's.
int mask_strides(const char *what, const int64_t *mask_ld, int64_t NC, int64_t ni, int64_t ld[3]) {
  ld[0] = 1, ld[1] = NC, ld[2] = NC * ni;
  for (int ax = 0; mask_ld && ax < 3; ++ax) {
    ld[ax] = mask_ld[ax];
    if (ld[ax] < 0)
      return fail(BLDP_EINVAL, "%smask stride %d is negative (%lld)", what, ax, (long long)ld[ax]);
  }
  return BLDP_OK;
}

// lowest element offset and byte length of a window's elements
void window_span(const Geo &g, int64_t *lo, size_t *bytes) {
  int64_t l = g.off, h = g.off;
  const int64_t span[3] = {(g.nc - 1) * g.cs, (g.ni - 1) * g.ld_i, (g.nt - 1) * g.ld_t};
  for (int ax = 0; ax < 3; ++ax) (span[ax] < 0 ? l : h) += span[ax];
  *lo = l;
  *bytes = 4 * (size_t)(h - l + 1);
}

bool spans_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

// The outputs (null ones skipped) may not overlap the window's elements of any
// bank, the mask's or profile's span `aux`, nor each other.
struct Span {
  const void *p;
  size_t bytes;
  const char *name;
};
int check_disjoint(const char *what, const Span *out, int nout, const Geo &g, int nbank,
                   const float *const *in, const Span &aux) {
  int64_t lo;
  size_t wbytes;
  window_span(g, &lo, &wbytes);
  for (int q = 0; q < nout; ++q) {
    if (!out[q].p) continue;
    for (int b = 0; b < nbank; ++b)
      if (spans_overlap(out[q].p, out[q].bytes, in[b] + lo, wbytes))
        return fail(BLDP_EINVAL, "%s%s overlaps the input window (bank %d)", what, out[q].name, b);
    if (spans_overlap(out[q].p, out[q].bytes, aux.p, aux.bytes))
      return fail(BLDP_EINVAL, "%s%s overlaps %s", what, out[q].name, aux.name);
  }
  for (int q = 0; q < nout; ++q)
    for (int r = q + 1; r < nout; ++r)
      if (out[q].p && out[r].p && spans_overlap(out[q].p, out[q].bytes, out[r].p, out[r].bytes))
        return fail(BLDP_EINVAL, "%s%s and %s overlap", what, out[q].name, out[r].name);
  return BLDP_OK;
}

int num_cus_current() {
  static std::mutex mu;
  static std::map<int, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  int n = 256;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    n = 256;
  cache[dev] = n;
  return n;
}

// log2 of the current device's XCD count for the per-XCD tile order
// (hipDeviceAttributeNumberOfXccs: 8 on an MI355X in SPX mode, fewer in the
// compute partitions), 0 when it is 1 or not a power of two.
int xcd_log2_current() {
  static std::mutex mu;
  static std::map<int, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  int n = 1, lg = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess) n = 1;
  (void)hipGetLastError();
  if (n > 1 && (n & (n - 1)) == 0)
    while ((1 << lg) < n) ++lg;
  cache[dev] = lg;
  return lg;
}

// Library-owned scratch, cached per (device, stream) so that concurrent
// streams never share a buffer.  Host threads sharing one stream (the GBT
// fan-out runs a thread per (worker, file) on torch's current stream) take
// turns: a call holds the entry's lock from the lookup until its last launch
// is queued, so its kernels sit back to back in the stream and the next
// call's kernels run after them.  Growing synchronizes the stream first.
struct Scratch {
  std::mutex mu;
  void *ptr = nullptr;
  size_t bytes = 0;
};
std::mutex g_ws_mu;
std::map<std::pair<int, void *>, Scratch> g_ws;

}  // namespace

int bldp::scratch_lease(hipStream_t s, size_t bytes, ScratchLease *lease) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  Scratch *w;
  {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    w = &g_ws[{dev, (void *)s}];  // map nodes are stable
  }
  std::unique_lock<std::mutex> hold(w->mu);
  if (w->bytes < bytes) {
    if (w->ptr) {
      HIPCHK(hipStreamSynchronize(s));  // earlier calls on this stream still use it
      HIPCHK(hipFree(w->ptr));
      w->ptr = nullptr;
      w->bytes = 0;
    }
    size_t want = std::max<size_t>(bytes, 1 << 20);
    if (hipMalloc(&w->ptr, want) != hipSuccess) {
      w->ptr = nullptr;
      return fail(BLDP_ENOMEM, "hipMalloc of %zu bytes of scratch failed", want);
    }
    w->bytes = want;
  }
  lease->ptr = w->ptr;
  lease->hold = std::move(hold);
  return BLDP_OK;
}

namespace {
// Staging of bldp_band_reduce_multi_f32's staged banks, one buffer per device
// (kept apart from the per-stream scratch, which the reduces of the same call
// may lease on the same stream).
struct StageBuf {
  std::mutex mu;
  void *ptr = nullptr;
  size_t bytes = 0;
};
std::mutex g_stage_mu;
std::map<int, StageBuf> g_stage;

// The current device's staging buffer of >= bytes, locked into *hold until
// the caller drops the lock (callers synchronize their work before that).
int staging_buffer(int dev, size_t bytes, void **ptr, std::vector<std::unique_lock<std::mutex>> *hold) {
  StageBuf *sb;
  {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    sb = &g_stage[dev];
  }
  std::unique_lock<std::mutex> lk(sb->mu);
  if (sb->bytes < bytes) {
    if (sb->ptr) (void)hipFree(sb->ptr);  // (no work in flight: calls synchronize)
    sb->ptr = nullptr;
    sb->bytes = 0;
    if (hipMalloc(&sb->ptr, bytes) != hipSuccess) {
      sb->ptr = nullptr;
      return fail(BLDP_ENOMEM, "staging allocation of %zu bytes on device %d failed", bytes, dev);
    }
    sb->bytes = bytes;
  }
  *ptr = sb->ptr;
  hold->push_back(std::move(lk));
  return BLDP_OK;
}
}  // namespace

std::vector<int> bldp::scratch_devices() {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  std::vector<int> d;
  for (auto &kv : g_ws) d.push_back(kv.first.first);
  return d;
}

void bldp::scratch_release_all() {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (auto &kv : g_ws) {
    std::lock_guard<std::mutex> hold(kv.second.mu);  // (callers drained the devices)
    if (kv.second.ptr) {
      (void)hipSetDevice(kv.first.first);
      (void)hipFree(kv.second.ptr);
    }
  }
  g_ws.clear();
  {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    for (auto &kv : g_stage) {
      std::lock_guard<std::mutex> hold(kv.second.mu);
      if (kv.second.ptr) {
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second.ptr);
      }
    }
    g_stage.clear();
  }
  if (prev >= 0) (void)hipSetDevice(prev);
}

namespace {

// Queue a planned operation on s: lease `ws_bytes` of scratch (held until
// `launch(workspace)` has queued every kernel) and record a failed launch.
template <class Launch>
int run_planned(const char *what, size_t ws_bytes, hipStream_t s, Launch launch) {
  ScratchLease lease;
  if (ws_bytes) {
    const int rc = scratch_lease(s, ws_bytes, &lease);
    if (rc) return rc;
  }
  const hipError_t e = launch(lease.ptr);
  if (e != hipSuccess) return fail(BLDP_EHIP, "%s launch: %s", what, hipGetErrorString(e));
  return BLDP_OK;
}

// The first eight words of a plan query over the reduce's plan and the tstat's.
void fill_reduce_info(int64_t *info, const Plan &p, const RedArgs &a) {
  info[0] = p.path, info[1] = p.lpg, info[2] = a.ts, info[3] = a.k4, info[4] = a.nchunk;
  info[5] = p.grid, info[6] = (int64_t)p.ws_bytes, info[7] = a.vec_out;
}
void fill_tstat_info(int64_t *info, const TStatPlan &p, const TStatArgs &a) {
  info[0] = p.path, info[1] = p.cpl, info[2] = p.tsplit, info[3] = p.passes;
  info[4] = p.grid, info[5] = (int64_t)p.ws_bytes, info[6] = a.nb;
  info[7] = p.tsplit > 1 ? ((int64_t)1 << a.lx_log2) : 0;
}

bool pitch_ok(const Geo &g) {
  return (g.ni <= 1 || g.ld_i % 4 == 0) && (g.nt <= 1 || g.ld_t % 4 == 0);
}
bool vec_ok(const Geo &g) { return g.cs == 1 && g.off % 4 == 0 && pitch_ok(g); }
// Unit-step windows that start off a 16-byte boundary (or have row pitches
// that are not multiples of 4 floats) on the vector paths (plan option
// "unaligned_vec"): gfx950 executes global_load_dwordx4 at any dword alignment
// (LLVM: unaligned-buffer-access), so the lanes load the window's own float4
// columns and no realignment is needed.  A/B on MI355X
// (profiles/r02/ab_unaligned_vec.json, 8 banks): c0=3 F=64 cfg3 5.42 -> 5.08
// ms, c0=1 F=8 T=1024 cfg4 3.30 -> 2.19 ms, c0=1 F=1 5.92 -> 5.78 ms; but
// c0=1/3 F=1024 4.92 -> 5.12 ms and c0=2 F=2 5.83 -> 6.03 ms (the tile /
// realigning kernels keep those); kurtosis c0=1 cfg4 5.79 -> 2.45 ms, cfg3
// 11.85 -> 6.64 ms (leaf / register paths instead of the two-pass / mid
// ones).  0 = off; 1 = reduce windows where it pays (below); 2 (default) =
// 1 + kurtosis.  (3, every unit-step reduce window: never won; removed in
// round 5.)
// A dword-aligned unit-step reduce window that is not 16-byte aligned goes to
// the vector / narrow paths when that measured faster than the realigning
// kernels, or when the alternative is the scalar path (pitches that are not
// multiples of 4 floats).
bool unaligned_vec_pays(int64_t F, bool rows16) {
  if (!rows16) return true;
  return F == 1 || (F % 4 == 0 && F <= 256);
}

int valid_op(int op) { return (op >= BLDP_OP_SUM && op <= BLDP_OP_MEDIAN) || op == BLDP_OP_MAD; }
#define BLDP_OP_NAMES "0=sum 1=mean 2=max 3=min 4=var 5=std 6=median 8=mad"

// Checks, window and plan of a reduce (shared by every reduce entry point and
// by the prepared form): fills *a and *p; *empty when there is nothing to do.
// qp: the probability of a quantile (the bldp_quantile_* entry points; op is
// then kOpQuantile, which no caller's op can be).  qset: the plan of
// bldp_quantiles_* (kOpQuantiles: the median's; the caller builds the QSet).
int prepare_reduce(int nbank, const float *const *in, int64_t nchan, int64_t nif, int64_t ntime,
                   const int64_t *win, int64_t fqavby, int64_t tavby, int op, float *out,
                   int64_t out_bank, int64_t out_ld_i, int64_t out_ld_t, bool stitched,
                   bool query, RedArgs *ap, Plan *pp, bool *empty, const double *qp = nullptr,
                   bool qset = false) {
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (qset)  // (the bldp_quantiles_* entry points: the ranks travel in a QSet)
    op = kOpQuantiles;
  else if (qp)
    op = kOpQuantile;
  else if (!valid_op(op))
    return fail(BLDP_EINVAL, "unknown op %d (" BLDP_OP_NAMES ")", op);
  const bool stat = stat_op(op) || qp || qset;
  // Statistics' var / std / median (and mad, quantile) reduce the channel blocks
  // only: fqav on the time axis after them would not be the statistic of the F x T block
  if (stat && tavby > 1)
    return fail(BLDP_EINVAL,
                "tavby=%lld: var/std/median/mad have no time integration (tavby <= 1)",
                (long long)tavby);
  Geo g;
  int64_t F, T;
  rc = resolve_blocks(nchan, nif, ntime, win, fqavby, tavby, &g, &F, &T);
  if (rc) return rc;
  RedArgs &a = *ap;
  a = RedArgs{};
  if (qp && F > 1) {
    int64_t q;
    quantile_rank(F, *qp, &q, &a.qg);
    a.qrank = (int32_t)q;
  }
  if (stitched) {
    const int64_t d[3] = {g.nc / F, g.ni, g.nt / T};
    vcat_layout(nbank, d, &out_bank, &out_ld_i, &out_ld_t);
  }
  *empty = set_blocks(a, g, F, T, out_bank, out_ld_i, out_ld_t);
  a.out = out;
  bool rows16, words;
  rc = set_window("", a, g, nbank, in, &words, &rows16);
  if (rc) return rc;
  rows16 = rows16 && pitch_ok(g);
  const bool aligned = (rows16 && vec_ok(g)) ||
                       (opt(OPT_UNALIGNED_VEC) >= 1 && words && g.cs == 1 &&
                        unaligned_vec_pays(F, rows16));
  if (stat) {
    rc = plan_stats(a, op, words && g.cs == 1, xcd_log2_current(), pp);
    if (rc) return rc;
  } else {
    *pp = plan_reduce(a, aligned, rows16, words && g.cs == 1, num_cus_current(),
                      xcd_log2_current());
  }
  if (query || *empty) return BLDP_OK;
  rc = check_banks("", nbank, in);
  if (rc) return rc;
  if (!out) return fail(BLDP_EINVAL, "null output pointer");
  return BLDP_OK;
}

// Queue a prepared reduce on stream s (scratch leased for time-chunk partials).
int run_reduce(RedArgs a, const Plan &p, int op, hipStream_t s) {
  return run_planned("reduce", p.ws_bytes, s, [&](void *ws) {
    if (ws) a.ws = (float *)ws;
    return stat_op(op) || op == kOpQuantile ? launch_stats(a, p, op, s)
                                            : launch_reduce(a, p, op, s);
  });
}

int reduce_impl(int nbank, const float *const *in, int64_t nchan, int64_t nif, int64_t ntime,
                const int64_t *win, int64_t fqavby, int64_t tavby, int op, float *out,
                int64_t out_bank, int64_t out_ld_i, int64_t out_ld_t, bool stitched,
                hipStream_t s, int64_t *info, const double *qp = nullptr) {
  RedArgs a;
  Plan p;
  bool empty = false;
  int rc = prepare_reduce(nbank, in, nchan, nif, ntime, win, fqavby, tavby, op, out, out_bank,
                          out_ld_i, out_ld_t, stitched, info != nullptr, &a, &p, &empty, qp);
  if (rc) return rc;
  if (qp) op = kOpQuantile;
  if (info) {
    fill_reduce_info(info, p, a);
    if (p.path == PATH_VEC_ROW) info[2] = a.rsplit;  // (k_reduce_rows: slices splitting T)
    if (qp) info[6] = a.F > 1 ? a.qrank : -1;  // (no workspace: the slot carries the lower rank)
    return BLDP_OK;  // plan query only
  }
  if (empty) return BLDP_OK;
  return run_reduce(a, p, op, s);
}

}  // namespace

extern "C" {

int bldp_abi_version(void) { return BLDP_ABI_VERSION; }

int bldp_last_error(char *buf, size_t len) {
  if (!buf || len == 0) return BLDP_EINVAL;
  std::snprintf(buf, len, "%s", g_err.c_str());
  return BLDP_OK;
}

int bldp_device_count(int *n) {
  if (!n) return fail(BLDP_EINVAL, "null pointer");
  HIPCHK(hipGetDeviceCount(n));
  return BLDP_OK;
}

int bldp_plan_option(const char *name, int64_t value, int64_t *previous) {
  if (!name) return fail(BLDP_EINVAL, "null option name");
  const int k = plan_opt_index(name);
  if (k < 0) return fail(BLDP_EINVAL, "unknown plan option '%s'", name);
  if (!plan_opt_valid(k, value)) {
    int64_t lo, hi;
    plan_opt_domain(k, &lo, &hi);
    return fail(BLDP_EINVAL, "plan option '%s' takes %s%lld..%lld or -1 (the default), not %lld",
                name, k == OPT_ROW_SPLIT ? "1, 2 or 4 in " : "", (long long)lo, (long long)hi,
                (long long)value);
  }
  if (previous) *previous = plan_opt_override(k);
  plan_opt_set(k, value < 0 ? -1 : value);
  return BLDP_OK;
}

int bldp_reduce_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                      int64_t fqavby, int64_t tavby, int64_t out_shape[3]) {
  if (!out_shape) return fail(BLDP_EINVAL, "null out_shape");
  Geo g;
  int64_t F, T;
  const int rc = resolve_blocks(nchan, nif, ntime, win, fqavby, tavby, &g, &F, &T);
  if (rc) return rc;
  out_shape[0] = g.nc / F;
  out_shape[1] = g.ni;
  out_shape[2] = g.nt / T;
  return BLDP_OK;
}

int bldp_reduce_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                         const int64_t *win, int64_t fqavby, int64_t tavby, int op,
                         const float *out, int64_t info[8]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  int64_t sh[3];
  int rc = bldp_reduce_shape(nchan, nif, ntime, win, fqavby, tavby, sh);
  if (rc) return rc;
  const float *ins[1] = {in};
  return reduce_impl(1, ins, nchan, nif, ntime, win, fqavby, tavby, op, (float *)out,
                     sh[0] * sh[1] * sh[2], sh[0], sh[0] * sh[1], false, nullptr, info);
}

int bldp_reduce_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, int64_t fqavby, int64_t tavby, int op, float *out,
                    void *stream) {
  int64_t sh[3];
  int rc = bldp_reduce_shape(nchan, nif, ntime, win, fqavby, tavby, sh);
  if (rc) return rc;
  const float *ins[1] = {in};
  return reduce_impl(1, ins, nchan, nif, ntime, win, fqavby, tavby, op, out,
                     sh[0] * sh[1] * sh[2], sh[0], sh[0] * sh[1], false, (hipStream_t)stream,
                     nullptr);
}

int bldp_reduce_strided_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                            const int64_t *win, int64_t fqavby, int64_t tavby, int op,
                            float *out, int64_t out_ld_i, int64_t out_ld_t, void *stream) {
  const float *ins[1] = {in};
  return reduce_impl(1, ins, nchan, nif, ntime, win, fqavby, tavby, op, out, 0, out_ld_i,
                     out_ld_t, false, (hipStream_t)stream, nullptr);
}

int bldp_band_reduce_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                         int op, float *out, void *stream) {
  return reduce_impl(nbank, in, nchan, nif, ntime, win, fqavby, tavby, op, out, 0, 0, 0, true,
                     (hipStream_t)stream, nullptr);
}

// A prepared band reduce: the checks, window, plan and kernel arguments of
// bldp_band_reduce_f32 computed once, so that a launch costs the host nothing
// but the kernel launch itself (a worker re-reducing the same buffers, bench
// loops).
struct bldp_reduce_op {
  // what a launch runs: a Float32 (band) reduce, a typed reduce, a typed
  // getkurtosis, a Float32 getkurtosis (bldp_reduce_prepare /
  // bldp_kurtosis_prepare prepare the last three)
  enum Kind { F32_REDUCE = 0, TYPED_REDUCE, TYPED_KURT, F32_KURT } kind = F32_REDUCE;
  RedArgs a;
  Plan p;
  bldp::TypedArgs t;
  bldp::KurtArgs k;
  double *kout = nullptr;
  int op;
  int dev;
  bool empty;
};

int bldp_band_reduce_prepare_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                 int64_t ntime, const int64_t *win, int64_t fqavby,
                                 int64_t tavby, int op, float *out, bldp_reduce_op_t *handle) {
  if (!handle) return fail(BLDP_EINVAL, "null handle pointer");
  *handle = nullptr;
  auto *h = new (std::nothrow) bldp_reduce_op{};
  if (!h) return fail(BLDP_ENOMEM, "out of host memory");
  int rc = prepare_reduce(nbank, in, nchan, nif, ntime, win, fqavby, tavby, op, out, 0, 0, 0,
                          true, false, &h->a, &h->p, &h->empty);
  if (rc == BLDP_OK && hipGetDevice(&h->dev) != hipSuccess)
    rc = fail(BLDP_EHIP, "hipGetDevice failed");
  if (rc) {
    delete h;
    return rc;
  }
  h->op = op;
  *handle = h;
  return BLDP_OK;
}

static int kurt_run(KurtArgs &k, double *out, void *workspace, void *stream);

namespace {
// Queue a prepared operation of any kind on s.
int run_prepared(bldp_reduce_op_t h, hipStream_t s) {
  switch (h->kind) {
    case bldp_reduce_op::F32_REDUCE: return run_reduce(h->a, h->p, h->op, s);
    case bldp_reduce_op::TYPED_REDUCE: {
      const hipError_t e = launch_reduce_typed(h->t, h->op, s);
      return e == hipSuccess ? BLDP_OK
                             : fail(BLDP_EHIP, "typed reduce launch: %s", hipGetErrorString(e));
    }
    case bldp_reduce_op::TYPED_KURT: {
      ScratchLease lease;  // time-chunk partial sums (k_kurt_i8), held until queued
      bldp::TypedArgs t = h->t;
      if (const size_t wsb = kurtosis_typed_ws_bytes(t)) {
        const int rc = scratch_lease(s, wsb, &lease);
        if (rc) return rc;
        t.ws = lease.ptr;
        t.ws_bytes = wsb;
      }
      const hipError_t e = launch_kurtosis_typed(t, h->kout, s);
      return e == hipSuccess ? BLDP_OK
                             : fail(BLDP_EHIP, "typed kurtosis launch: %s", hipGetErrorString(e));
    }
    case bldp_reduce_op::F32_KURT: return kurt_run(h->k, h->kout, nullptr, s);
  }
  return fail(BLDP_EINVAL, "bad prepared operation");
}
}  // namespace

int bldp_reduce_launch(bldp_reduce_op_t h, void *stream) {
  if (!h) return fail(BLDP_EINVAL, "null reduce handle");
  if (h->empty) return BLDP_OK;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != h->dev)
    return fail(BLDP_EINVAL, "reduce handle prepared on device %d, current device %d", h->dev,
                dev);
  return run_prepared(h, (hipStream_t)stream);
}

int bldp_reduce_launch_timed(bldp_reduce_op_t h, void *stream, void *ev_start, void *ev_stop) {
  if (!h) return fail(BLDP_EINVAL, "null reduce handle");
  if (!ev_start || !ev_stop) return fail(BLDP_EINVAL, "null timing event");
  if (h->empty) return BLDP_OK;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != h->dev)
    return fail(BLDP_EINVAL, "reduce handle prepared on device %d, current device %d", h->dev,
                dev);
  if (h->kind != bldp_reduce_op::F32_REDUCE) {  // events recorded around the launch
    if (hipEventRecord((hipEvent_t)ev_start, (hipStream_t)stream) != hipSuccess)
      return fail(BLDP_EHIP, "hipEventRecord failed");
    const int rc = run_prepared(h, (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(hipEventRecord((hipEvent_t)ev_stop, (hipStream_t)stream));
    return BLDP_OK;
  }
  set_launch_events((hipEvent_t)ev_start, (hipEvent_t)ev_stop);
  const int rc = run_prepared(h, (hipStream_t)stream);
  set_launch_events(nullptr, nullptr);
  return rc;
}

int bldp_reduce_release(bldp_reduce_op_t h) {
  delete h;
  return BLDP_OK;
}

int bldp_peer_access(int dev, int peer, int *direct) {
  if (!direct) return fail(BLDP_EINVAL, "null pointer");
  *direct = 0;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (dev < 0 || dev >= ndev || peer < 0 || peer >= ndev)
    return fail(BLDP_EINVAL, "device %d / peer %d not available (%d visible)", dev, peer, ndev);
  if (dev == peer) {
    *direct = 1;
    return BLDP_OK;
  }
  int can = 0;
  if (hipDeviceCanAccessPeer(&can, dev, peer) != hipSuccess || !can) {
    (void)hipGetLastError();
    return BLDP_OK;
  }
  int prev = 0;
  HIPCHK(hipGetDevice(&prev));
  HIPCHK(hipSetDevice(dev));
  const hipError_t pe = hipDeviceEnablePeerAccess(peer, 0);
  (void)hipGetLastError();
  (void)hipSetDevice(prev);
  *direct = pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled;
  return BLDP_OK;
}

int bldp_band_reduce_multi_f32(int nbank, const int *bank_dev, const float *const *in,
                               int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                               int64_t fqavby, int64_t tavby, int op, int root, float *out,
                               unsigned flags) {
  if (nbank < 1 || nbank > BLDP_MAX_BANKS || !bank_dev || !in)
    return fail(BLDP_EINVAL, "bad bank arguments");
  if (stat_op(op))
    return fail(BLDP_EINVAL, "var/std/median/mad (op %d) run on one device: reduce each device's "
                             "banks with bldp_band_reduce_f32", op);
  if (flags & ~(BLDP_BAND_STAGED | BLDP_BAND_PEER_STORE))
    return fail(BLDP_EINVAL, "unknown flags 0x%x", flags);
  if ((flags & BLDP_BAND_STAGED) && (flags & BLDP_BAND_PEER_STORE))
    return fail(BLDP_EINVAL, "BLDP_BAND_STAGED and BLDP_BAND_PEER_STORE exclude each other");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (root < 0 || root >= ndev) return fail(BLDP_EINVAL, "root device %d not available", root);
  for (int b = 0; b < nbank; ++b)
    if (bank_dev[b] < 0 || bank_dev[b] >= ndev)
      return fail(BLDP_EINVAL, "bank %d: device %d not available", b, bank_dev[b]);
  int64_t sh[3];
  int rc = bldp_reduce_shape(nchan, nif, ntime, win, fqavby, tavby, sh);
  if (rc) return rc;
  const int64_t nco = sh[0], ni = sh[1], nto = sh[2];
  if (nco * ni * nto == 0) return BLDP_OK;
  if (!out) return fail(BLDP_EINVAL, "null output pointer");
  const int64_t ld_i = (int64_t)nbank * nco, ld_t = ld_i * ni;
  // BLDP_BAND_STAGED: every bank takes the staged branch (local reduce +
  // strided copy into the root's slot), even on the root device
  const bool force_staged = (flags & BLDP_BAND_STAGED) != 0;
  const bool peer_store = (flags & BLDP_BAND_PEER_STORE) != 0;
  int prev = 0;
  HIPCHK(hipGetDevice(&prev));
  // A device's banks, in bank order, cut into runs whose bank indices step
  // evenly (b0, b0 + s, b0 + 2s, ...): one reduce launch per run, its banks'
  // vcat slots nco * s floats apart.  Contiguous bank-per-device shards (GBT's
  // workers, bench.py's ranks) are one run, i.e. one launch per device.
  struct Run {
    int dev, nb, step;
    int bank[BLDP_MAX_BANKS];
    bool direct;
    size_t stage_off;  // staged runs: floats into the device's staging buffer
  };
  std::vector<Run> runs;
  std::vector<size_t> nstaged(ndev, 0);  // floats of staging per device
  std::vector<hipStream_t> streams(ndev, nullptr);
  const size_t per = (size_t)(nco * ni * nto);
  for (int d = 0; d < ndev && rc == BLDP_OK; ++d) {
    std::vector<int> mine;
    for (int b = 0; b < nbank; ++b)
      if (bank_dev[b] == d) mine.push_back(b);
    if (mine.empty()) continue;
    if ((rc = device_stream(d, &streams[d])) != BLDP_OK) break;
    // the root stores its own slots; another device only with
    // BLDP_BAND_PEER_STORE and peer access (kernel stores over xGMI), else
    // its runs are reduced into staging on the device and DMA-copied
    bool dir = d == root && !force_staged;
    if (!dir && peer_store) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, d, root) == hipSuccess && can) {
        if (hipSetDevice(d) != hipSuccess) {
          rc = fail(BLDP_EHIP, "hipSetDevice(%d) failed", d);
          break;
        }
        const hipError_t pe = hipDeviceEnablePeerAccess(root, 0);
        dir = pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled;
      }
      (void)hipGetLastError();
    }
    for (size_t i = 0; i < mine.size();) {
      Run r{};
      r.dev = d;
      r.direct = dir;
      r.bank[0] = mine[i];
      r.nb = 1;
      r.step = i + 1 < mine.size() ? mine[i + 1] - mine[i] : 1;
      while (i + r.nb < mine.size() && mine[i + r.nb] - mine[i + r.nb - 1] == r.step) {
        r.bank[r.nb] = mine[i + r.nb];
        ++r.nb;
      }
      i += r.nb;
      if (!dir) {
        r.stage_off = nstaged[d];
        nstaged[d] += per * r.nb;
      }
      runs.push_back(r);
    }
  }
  // staging: a library-owned buffer per device (no allocation per call once
  // it has grown), held until every launch and copy of this call is done
  // (the call synchronizes before it returns)
  std::vector<std::unique_lock<std::mutex>> hold;
  std::vector<void *> stage(ndev, nullptr);
  for (int d = 0; d < ndev && rc == BLDP_OK; ++d)
    if (nstaged[d]) {
      if (hipSetDevice(d) != hipSuccess) {
        rc = fail(BLDP_EHIP, "hipSetDevice(%d) failed", d);
        break;
      }
      rc = staging_buffer(d, nstaged[d] * sizeof(float), &stage[d], &hold);
    }
  for (const Run &r : runs) {
    if (rc != BLDP_OK) break;
    if (hipSetDevice(r.dev) != hipSuccess) {
      rc = fail(BLDP_EHIP, "hipSetDevice(%d) failed", r.dev);
      break;
    }
    const float *ins[BLDP_MAX_BANKS];
    for (int j = 0; j < r.nb; ++j) ins[j] = in[r.bank[j]];
    if (r.direct) {  // one launch: the run's banks into their slots of the root's product
      rc = reduce_impl(r.nb, ins, nchan, nif, ntime, win, fqavby, tavby, op,
                       out + (int64_t)r.bank[0] * nco, (int64_t)r.step * nco, ld_i, ld_t, false,
                       streams[r.dev], nullptr);
      continue;
    }
    // one launch into staging (the run's banks stitched among themselves),
    // then strided copies into the root's slots: one 2-D copy for a run of
    // neighbouring banks, one per bank otherwise
    float *st = (float *)stage[r.dev] + r.stage_off;
    const int64_t sld_i = (int64_t)r.nb * nco;
    rc = reduce_impl(r.nb, ins, nchan, nif, ntime, win, fqavby, tavby, op, st, nco, sld_i,
                     sld_i * ni, false, streams[r.dev], nullptr);
    const int ncopy = r.step == 1 ? 1 : r.nb;
    const int64_t width = r.step == 1 ? sld_i : nco;
    for (int j = 0; j < ncopy && rc == BLDP_OK; ++j)
      if (hipMemcpy2DAsync(out + (int64_t)r.bank[j] * nco, ld_i * sizeof(float), st + j * nco,
                           sld_i * sizeof(float), width * sizeof(float), (size_t)(ni * nto),
                           hipMemcpyDeviceToDevice, streams[r.dev]) != hipSuccess)
        rc = fail(BLDP_EHIP, "peer copy of bank %d failed", r.bank[j]);
  }
  for (int d = 0; d < ndev; ++d)
    if (streams[d]) {
      (void)hipSetDevice(d);
      if (hipStreamSynchronize(streams[d]) != hipSuccess && rc == BLDP_OK)
        rc = fail(BLDP_EHIP, "device %d failed during the band reduce", d);
    }
  (void)hipSetDevice(prev);
  return rc;
}

int bldp_stitch_f32(int nbank, const float *gathered, int64_t nc, int64_t nif, int64_t ntime,
                    float *out, void *stream) {
  if (check_nbank(nbank)) return BLDP_EINVAL;
  if (nc < 0 || nif < 0 || ntime < 0) return fail(BLDP_EINVAL, "negative dimension");
  const int64_t n = nc * nif * ntime;
  if (n > 0 && (!gathered || !out)) return fail(BLDP_EINVAL, "null pointer");
  if (n > 0 && gathered == out) return fail(BLDP_EINVAL, "stitch cannot run in place");
  hipError_t e = launch_stitch(nbank, gathered, nc, nif * ntime, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(BLDP_EHIP, "stitch launch: %s", hipGetErrorString(e));
  return BLDP_OK;
}

int bldp_despike_f32(float *data, int64_t nchan, int64_t nif, int64_t ntime, int64_t nfpc,
                     void *stream) {
  if (nchan < 0 || nif < 0 || ntime < 0) return fail(BLDP_EINVAL, "negative dimension");
  // spike = nfpc÷2 + 1 (1-based, src/gbt.jl:102); spike-1 must be a valid index
  if (nfpc < 2) return fail(BLDP_EBOUNDS, "BoundsError: nfpc=%lld < 2", (long long)nfpc);
  const int64_t sp = nfpc / 2;  // 0-based spike bin
  const int64_t nspike = nchan > sp ? (nchan - sp + nfpc - 1) / nfpc : 0;
  const int64_t nsrc = nchan > sp - 1 ? (nchan - (sp - 1) + nfpc - 1) / nfpc : 0;
  if (nspike != nsrc)  // d[spike:nfpc:end] .= d[spike-1:nfpc:end] length mismatch
    return fail(BLDP_EDIM,
                "DimensionMismatch: %lld spike bins vs %lld source bins (nchan=%lld, nfpc=%lld)",
                (long long)nspike, (long long)nsrc, (long long)nchan, (long long)nfpc);
  if (nspike * nif * ntime > 0 && !data) return fail(BLDP_EINVAL, "null pointer");
  hipError_t e = launch_despike(data, nchan, nif * ntime, nfpc, nspike, (hipStream_t)stream);
  if (e != hipSuccess) return fail(BLDP_EHIP, "despike launch: %s", hipGetErrorString(e));
  return BLDP_OK;
}

// `order`: the moment of the plan, 4 = kurtosis, 3 = skewness (bldp_skewness_*),
// kOrdAll = every plane of KurtArgs.mo (bldp_moments_*)
static bool any_plane(double *const *mo) { return mo && (mo[0] || mo[1] || mo[2] || mo[3]); }
static int kurt_setup(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                      int64_t ntime, const int64_t *win, KurtArgs *k, int order) {
  if (check_nbank(nbank)) return BLDP_EINVAL;
  Geo g;
  int rc = resolve_window(nchan, nif, ntime, win, &g);
  if (rc) return rc;
  *k = KurtArgs{};
  k->order = order;
  k->nbank = nbank;
  bool aligned = true, words = true;
  for (int b = 0; b < nbank; ++b) {
    k->in[b] = in ? in[b] : nullptr;
    aligned = aligned && aligned16(k->in[b]);
    words = words && aligned4(k->in[b]);
  }
  k->in_off = g.off;
  k->in_cs = g.cs;
  k->in_ld_i = g.ld_i;
  k->in_ld_t = g.ld_t;
  k->nc = g.nc;
  k->ni = g.ni;
  k->nt = g.nt;
  k->nrow = (int64_t)nbank * g.ni;
  k->rows16 = vec_ok(g) && g.nc % 4 == 0 && aligned;
  k->vec = opt(OPT_UNALIGNED_VEC) >= 2 ? (g.cs == 1 && g.nc % 4 == 0 && words) : k->rows16;
  plan_kurtosis(*k, num_cus_current());
  return BLDP_OK;
}

// (order kOrdAll: the caller has set k.mo, `out` is not read)
static int kurt_run(KurtArgs &k, double *out, void *workspace, void *stream) {
  if (k.nc * k.nrow == 0) return BLDP_OK;
  if (kurtosis_max_grid(k) > INT32_MAX)
    return fail(BLDP_EINVAL, "kurtosis window too large for one launch");
  for (int b = 0; b < k.nbank; ++b)
    if (!k.in[b] && k.nt > 0) return fail(BLDP_EINVAL, "null input pointer (bank %d)", b);
  if (k.order == kOrdAll ? !any_plane(k.mo) : !out)
    return fail(BLDP_EINVAL, "null output pointer");
  k.out = out;
  hipStream_t s = (hipStream_t)stream;
  void *ws = workspace;
  ScratchLease lease;  // held until the launches are queued
  if (!ws) {
    int rc = scratch_lease(s, kurtosis_ws_bytes(k), &lease);
    if (rc) return rc;
    ws = lease.ptr;
  }
  hipError_t e = launch_kurtosis(k, (char *)ws, s);
  if (e != hipSuccess) return fail(BLDP_EHIP, "kurtosis launch: %s", hipGetErrorString(e));
  return BLDP_OK;
}

size_t bldp_kurtosis_workspace_size(int64_t nchan, int64_t nif, int64_t ntime,
                                    const int64_t *win) {
  KurtArgs k;
  const float *none[1] = {nullptr};
  if (kurt_setup(1, none, nchan, nif, ntime, win, &k, 4)) return 0;
  // enough for either plan: the path depends on the pointer's alignment
  k.vec = 1;
  const size_t a = kurtosis_ws_bytes(k);
  k.vec = 0;
  return std::max(a, kurtosis_ws_bytes(k));
}

int bldp_kurtosis_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, int64_t info[4]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  KurtArgs k;
  const float *ins[1] = {in};
  int rc = kurt_setup(1, ins, nchan, nif, ntime, win, &k, 4);
  if (rc) return rc;
  info[0] = kurtosis_path(k);
  info[1] = k.K;
  info[2] = k.nslot;
  info[3] = (int64_t)kurtosis_ws_bytes(k);
  return BLDP_OK;
}

int bldp_kurtosis_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                      const int64_t *win, double *out, void *workspace, void *stream) {
  KurtArgs k;
  const float *ins[1] = {in};
  int rc = kurt_setup(1, ins, nchan, nif, ntime, win, &k, 4);
  if (rc) return rc;
  return kurt_run(k, out, workspace, stream);
}

int bldp_band_kurtosis_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                           int64_t ntime, const int64_t *win, double *out, void *stream) {
  if (!in) return fail(BLDP_EINVAL, "null input pointer array");
  KurtArgs k;
  int rc = kurt_setup(nbank, in, nchan, nif, ntime, win, &k, 4);
  if (rc) return rc;
  return kurt_run(k, out, nullptr, stream);
}

// ---- the time-moment family: kurtosis over blocks, skewness, moments ---------
// One planner and one runner for (order, tblock); tblock = 0 is the whole
// window (one block of every selected spectrum), tblock >= 1 every block of
// tblock spectra.  The kernels, paths and workspace are the kurtosis' with
// KurtArgs.order = 3 (getskewness) or kOrdAll (getmoments: four planes that
// share their strides, a null plane is skipped).
struct MomKind {
  int order;         // 4, 3 or kOrdAll
  const char *what;  // prefix of the entries' messages
  bool whole_ok;     // tblock = 0 allowed (bldp_kurtosis_blocks_* take tblock >= 1)
};
static const MomKind kKurtBlocks{4, "tblock kurtosis", false};
static const MomKind kSkewness{3, "skewness", true};
static const MomKind kMoments{kOrdAll, "moments", true};

// Where a call's results go: element (c, i, b) of bank k at plane[q][k*out_bank
// + c + i*ld_i + b*ld_b]; orders 3 and 4 use plane[0], kOrdAll the four of
// KurtArgs.mo.  `dense` (the band entries): [nbank][nb][ni][nc], the strides
// follow from the window.
struct MomOut {
  double *plane[4];
  bool dense;
  int64_t ld_i, ld_b;
};

// The rule tavby follows: tblock must divide the selected spectra.
static int kblk_count(int64_t nt, int64_t tblock, int64_t *nb) {
  if (tblock < 1) return fail(BLDP_EINVAL, "tblock=%lld must be >= 1", (long long)tblock);
  if (nt % tblock != 0)
    return fail(BLDP_EDIM, "DimensionMismatch: tblock=%lld does not divide ntime=%lld",
                (long long)tblock, (long long)nt);
  *nb = nt / tblock;
  return BLDP_OK;
}

static int mom_tblock(const MomKind &c, int64_t tblock) {
  if (c.whole_ok && tblock < 0)
    return fail(BLDP_EINVAL, "%s: tblock=%lld must be >= 0", c.what, (long long)tblock);
  return BLDP_OK;
}

// The (nc, ni, nb) of a result.
static int mom_dims(const MomKind &c, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, int64_t tblock, int64_t dims[3]) {
  Geo g;
  int rc = resolve_window(nchan, nif, ntime, win, &g);
  if (rc) return rc;
  int64_t nb = 1;
  if (tblock > 0 || !c.whole_ok) {
    rc = kblk_count(g.nt, tblock, &nb);
    if (rc) return rc;
  }
  dims[0] = g.nc;
  dims[1] = g.ni;
  dims[2] = nb;
  return BLDP_OK;
}

// The window of block b: the same channels and IFs, spectra [b*M, (b+1)*M) of
// the selected ones.
static void kblk_window(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int64_t M,
                        int64_t b, int64_t bw[9]) {
  const int64_t full[9] = {0, nchan, 1, 0, nif, 1, 0, ntime, 1};
  for (int q = 0; q < 9; ++q) bw[q] = win ? win[q] : full[q];
  bw[6] += b * M * bw[8];
  bw[7] = M;
}

// Plan of a call: *whole is the whole window's KurtArgs (checks, float4
// columns), *blk the first block's (the block-by-block form's path and
// workspace; every block has the same shape; tblock = 0: the whole window).
struct MomPlan {
  KurtArgs whole, blk;
  int64_t nb;
  bool fused;  // the one-launch kernel over every block
  int path;
  // block by block: a block's dense results after its workspace.  ws_bytes is
  // what the plan entries report: with tblock the workspace and those results,
  // without one the workspace alone (a dense result needs no more).
  size_t tmp_off, ws_bytes;
};
static int mom_plan(const MomKind &c, int nbank, const float *const *in, int64_t nchan,
                    int64_t nif, int64_t ntime, const int64_t *win, int64_t tblock, MomPlan *p) {
  int rc = kurt_setup(nbank, in, nchan, nif, ntime, win, &p->whole, c.order);
  if (rc) return rc;
  p->nb = 1;
  if (tblock > 0 || !c.whole_ok) {
    rc = kblk_count(p->whole.nt, tblock, &p->nb);
    if (rc) return rc;
  }
  p->fused = tblock > 0 && kurt_blocks_fused(p->whole, tblock);
  p->tmp_off = p->ws_bytes = 0;
  if (p->fused) {
    p->path = tblock <= 32 ? 0 : 2;  // regs : leaf (KURT_PATHS)
    return BLDP_OK;
  }
  p->blk = p->whole;
  if (tblock > 0) {
    int64_t bw[9];
    kblk_window(nchan, nif, ntime, win, tblock, 0, bw);
    if (p->nb == 0) bw[6] = 0, bw[7] = 0;  // (no block: the empty window's plan)
    rc = kurt_setup(nbank, in, nchan, nif, ntime, bw, &p->blk, c.order);
    if (rc) return rc;
  }
  p->path = kurtosis_path(p->blk);
  p->ws_bytes = kurtosis_ws_bytes(p->blk);
  p->tmp_off = (p->ws_bytes + 255) & ~(size_t)255;
  // (order kOrdAll stages up to four planes of a block)
  if (tblock > 0)
    p->ws_bytes = p->tmp_off + (c.order == kOrdAll ? 4 : 1) *
                                   (size_t)(p->blk.nrow * p->blk.nc) * sizeof(double);
  return BLDP_OK;
}

// The four words of bldp_kurtosis_blocks_plan_f32 / _skewness_ / _moments_.
static int mom_plan_info(const MomKind &c, const float *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int64_t tblock, int64_t info[4]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  int rc = mom_tblock(c, tblock);
  if (rc) return rc;
  MomPlan p;
  const float *ins[1] = {in};
  rc = mom_plan(c, 1, ins, nchan, nif, ntime, win, tblock, &p);
  if (rc) return rc;
  info[0] = p.path;
  info[1] = tblock == 0 || p.fused ? 1 : 0;  // (the window: one set of launches)
  info[2] = p.nb;
  info[3] = (int64_t)p.ws_bytes;
  return BLDP_OK;
}

// Moments only: the planes may not overlap each other or the input array.
// `span` elements from each plane's pointer hold its result, `in_elems` floats
// each bank's array.
static int mom_check(int nbank, const float *const *in, int64_t in_elems, double *const mo[4],
                     int64_t span) {
  if (!any_plane(mo)) return fail(BLDP_EINVAL, "moments: every output plane is null");
  const size_t pb = (size_t)span * sizeof(double), ib = (size_t)in_elems * sizeof(float);
  for (int q = 0; q < 4; ++q) {
    if (!mo[q]) continue;
    for (int r = q + 1; r < 4; ++r)
      if (mo[r] && spans_overlap(mo[q], pb, mo[r], pb))
        return fail(BLDP_EINVAL, "moments: output planes %d and %d overlap", q, r);
    for (int b = 0; b < nbank; ++b)
      if (in[b] && spans_overlap(mo[q], pb, in[b], ib))
        return fail(BLDP_EINVAL, "moments: output plane %d overlaps the input (bank %d)", q, b);
  }
  return BLDP_OK;
}

// Every device entry of the family: each argument check once, then the run.
static int mom_run(const MomKind &c, const MomOut &o, int nbank, const float *const *in,
                   int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int64_t tblock,
                   void *stream) {
  const bool all = c.order == kOrdAll;
  const int np = all ? 4 : 1;
  int rc = mom_tblock(c, tblock);
  if (rc) return rc;
  if (!in) return fail(BLDP_EINVAL, "%s: null input pointer array", c.what);
  if (o.dense && !all) {
    // (the band kurtosis and skewness answer a bad window or tblock before a
    // bad nbank, the moments after it)
    int64_t d[3];
    rc = mom_dims(c, nchan, nif, ntime, win, tblock, d);
    if (rc) return rc;
  }
  MomPlan p;
  rc = mom_plan(c, nbank, in, nchan, nif, ntime, win, tblock, &p);
  if (rc) return rc;
  const KurtArgs &w = p.whole;
  if (w.nc * w.ni * p.nb == 0) return BLDP_OK;
  for (int b = 0; b < nbank; ++b)
    if (!w.in[b] && w.nt > 0)
      return fail(BLDP_EINVAL, "%s: null input pointer (bank %d)", c.what, b);
  if (!all && !o.plane[0]) return fail(BLDP_EINVAL, "%s: null output pointer", c.what);
  const int64_t out_ld_i = o.dense ? w.nc : o.ld_i;
  const int64_t out_ld_b = o.dense ? w.nc * w.ni : o.ld_b;
  const int64_t out_bank = o.dense ? w.nc * w.ni * p.nb : 0;
  if (out_ld_i < w.nc || (tblock > 0 && out_ld_b < (w.ni - 1) * out_ld_i + w.nc)) {
    if (tblock == 0 && !all)  // (the whole-window skewness names the bank stride)
      return fail(BLDP_EINVAL, "%s: out strides (%lld, %lld) overlap for a (%lld, %lld) result",
                  c.what, (long long)out_ld_i, (long long)out_bank, (long long)w.nc,
                  (long long)w.ni);
    return fail(BLDP_EINVAL,
                "%s: out strides (%lld, %lld) overlap for a (%lld, %lld, %lld) result", c.what,
                (long long)out_ld_i, (long long)out_ld_b, (long long)w.nc, (long long)w.ni,
                (long long)p.nb);
  }
  if (all) {
    const int64_t span = (nbank - 1) * out_bank + (tblock > 0 ? (p.nb - 1) * out_ld_b : 0) +
                         (w.ni - 1) * out_ld_i + w.nc;
    rc = mom_check(nbank, in, nchan * nif * ntime, o.plane, span);
    if (rc) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  if (p.fused) {
    KurtBlkArgs k{};
    for (int b = 0; b < nbank; ++b) k.in[b] = w.in[b];
    k.nbank = nbank;
    k.in_off = w.in_off;
    k.in_ld_i = w.in_ld_i;
    k.in_ld_t = w.in_ld_t;
    k.nc = w.nc;
    k.ni = w.ni;
    k.M = tblock;
    k.nb = p.nb;
    k.out_bank = out_bank;
    k.out_ld_i = out_ld_i;
    k.out_ld_b = out_ld_b;
    k.order = c.order;
    if (all)
      for (int q = 0; q < 4; ++q) k.mo[q] = o.plane[q];
    else
      k.out = o.plane[0];
    plan_kurt_blocks(k, num_cus_current());
    if (kurt_blocks_grid(k) > INT32_MAX)
      return fail(BLDP_EINVAL, "tblock=%lld kurtosis: %lld blocks are too many for one launch",
                  (long long)tblock, (long long)p.nb);
    hipError_t e = launch_kurt_blocks(k, s);
    if (e != hipSuccess)
      return fail(BLDP_EHIP, "%s launch: %s", c.what, hipGetErrorString(e));
    return BLDP_OK;
  }
  // Block by block through the whole-window paths: one scratch lease, every
  // launch on the caller's stream (which orders the reuse of the scratch).
  // Where a block's results are dense in the planes the kernels write them;
  // elsewhere they go to the scratch and are scattered.
  const bool direct =
      out_ld_i == w.nc && (nbank == 1 || (tblock == 0 && out_bank == w.nc * w.ni));
  if (tblock == 0 && direct) {
    // A dense whole window needs the workspace alone, and kurt_run leases it.
    // (A lease taken here may be empty, the regs path has no workspace:
    // kurt_run would then lease the entry this call holds.)
    KurtArgs k = p.blk;
    for (int q = 0; all && q < 4; ++q) k.mo[q] = o.plane[q];
    return kurt_run(k, all ? nullptr : o.plane[0], nullptr, stream);
  }
  const int64_t n = p.blk.nrow * p.blk.nc;
  ScratchLease lease;  // never empty (n > 0); held until the launches are queued
  rc = scratch_lease(s, p.tmp_off + np * (size_t)n * sizeof(double), &lease);
  if (rc) return rc;
  char *ws = static_cast<char *>(lease.ptr);
  double *tmp = reinterpret_cast<double *>(ws + p.tmp_off);
  for (int64_t b = 0; b < p.nb; ++b) {
    KurtArgs k = p.blk;
    if (b > 0) {
      int64_t bw[9];
      kblk_window(nchan, nif, ntime, win, tblock, b, bw);
      rc = kurt_setup(nbank, in, nchan, nif, ntime, bw, &k, c.order);
      if (rc) return rc;
      if (kurtosis_ws_bytes(k) > p.tmp_off)  // (a plan option changed under the call)
        return fail(BLDP_EINVAL, "%s: the plan changed during the call", c.what);
    }
    double *dst[4];  // where the kernels write this block's planes
    for (int q = 0; q < np; ++q)
      dst[q] = !o.plane[q] ? nullptr : direct ? o.plane[q] + b * out_ld_b : tmp + q * n;
    for (int q = 0; all && q < 4; ++q) k.mo[q] = dst[q];
    rc = kurt_run(k, all ? nullptr : dst[0], ws, stream);
    if (rc) return rc;
    for (int q = 0; !direct && q < np; ++q) {
      if (!o.plane[q]) continue;
      hipError_t e = launch_kurt_scatter(dst[q], nbank, w.ni, w.nc, o.plane[q] + b * out_ld_b,
                                         out_bank, out_ld_i, s);
      if (e != hipSuccess)
        return fail(BLDP_EHIP, "%s launch: %s", c.what, hipGetErrorString(e));
    }
  }
  return BLDP_OK;
}

int bldp_kurtosis_blocks_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                               int64_t tblock, int64_t dims[3]) {
  if (!dims) return fail(BLDP_EINVAL, "null dims");
  return mom_dims(kKurtBlocks, nchan, nif, ntime, win, tblock, dims);
}

int bldp_kurtosis_blocks_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                  const int64_t *win, int64_t tblock, int64_t info[4]) {
  return mom_plan_info(kKurtBlocks, in, nchan, nif, ntime, win, tblock, info);
}

int bldp_skewness_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, int64_t tblock, int64_t info[4]) {
  return mom_plan_info(kSkewness, in, nchan, nif, ntime, win, tblock, info);
}

int bldp_moments_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                          const int64_t *win, int64_t tblock, int64_t info[4]) {
  return mom_plan_info(kMoments, in, nchan, nif, ntime, win, tblock, info);
}

int bldp_kurtosis_blocks_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                             const int64_t *win, int64_t tblock, double *out, int64_t out_ld_i,
                             int64_t out_ld_b, void *stream) {
  const float *ins[1] = {in};
  return mom_run(kKurtBlocks, {{out}, false, out_ld_i, out_ld_b}, 1, ins, nchan, nif, ntime,
                 win, tblock, stream);
}

int bldp_band_kurtosis_blocks_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, int64_t tblock, double *out,
                                  void *stream) {
  return mom_run(kKurtBlocks, {{out}, true}, nbank, in, nchan, nif, ntime, win, tblock,
                 stream);
}

int bldp_skewness_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                      const int64_t *win, int64_t tblock, double *out, int64_t out_ld_i,
                      int64_t out_ld_b, void *stream) {
  const float *ins[1] = {in};
  return mom_run(kSkewness, {{out}, false, out_ld_i, out_ld_b}, 1, ins, nchan, nif, ntime,
                 win, tblock, stream);
}

int bldp_band_skewness_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                           int64_t ntime, const int64_t *win, int64_t tblock, double *out,
                           void *stream) {
  return mom_run(kSkewness, {{out}, true}, nbank, in, nchan, nif, ntime, win, tblock, stream);
}

int bldp_moments_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                     const int64_t *win, int64_t tblock, double *mean, double *var, double *skew,
                     double *kurt, int64_t out_ld_i, int64_t out_ld_b, void *stream) {
  const float *ins[1] = {in};
  return mom_run(kMoments, {{mean, var, skew, kurt}, false, out_ld_i, out_ld_b}, 1, ins,
                 nchan, nif, ntime, win, tblock, stream);
}

int bldp_band_moments_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                          int64_t ntime, const int64_t *win, int64_t tblock, double *mean,
                          double *var, double *skew, double *kurt, void *stream) {
  return mom_run(kMoments, {{mean, var, skew, kurt}, true}, nbank, in, nchan, nif, ntime, win,
                 tblock, stream);
}

// ---- tavfunc: median / var / std over blocks of spectra ---------------------
// Checks, window and plan of a tstat (every entry point): *copy when tavby <= 1
// (fqav's n <= 1 rule: the window itself, whatever the op).
static int tstat_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int64_t tavby, int op, float *out,
                         int64_t out_bank, int64_t out_ld_i, int64_t out_ld_b, bool query,
                         TStatArgs *ap, TStatPlan *pp, bool *copy, bool *empty,
                         const double *qp = nullptr) {
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (qp)  // (the bldp_quantile_* entry points: kOpQuantile, which no caller's op can be)
    op = kOpQuantile;
  else if (!stat_op(op))
    return fail(BLDP_EINVAL,
                "tstat: op %d is not 4=var 5=std 6=median 8=mad (sum/mean/max/min over time: "
                "bldp_reduce_* with tavby)",
                op);
  Geo g;
  int64_t F, T;
  rc = resolve_blocks(nchan, nif, ntime, win, 1, tavby, &g, &F, &T);
  if (rc) return rc;
  *copy = T <= 1;
  TStatArgs &a = *ap;
  a = TStatArgs{};
  a.nc = g.nc;
  a.ni = g.ni;
  a.T = T;
  a.nb = g.nt / T;
  a.out = out;
  a.out_bank = out_bank;
  a.out_ld_i = out_ld_i;
  a.out_ld_b = out_ld_b;
  if (qp && T > 1) {
    int64_t q;
    quantile_rank(T, *qp, &q, &a.qg);
    a.qrank = (int32_t)q;
  }
  *empty = a.nc == 0 || a.ni == 0 || a.nb == 0;
  bool words;
  rc = set_window("tstat: ", a, g, nbank, in, &words);
  if (rc) return rc;
  *pp = TStatPlan{};
  if (!*copy) {
    rc = plan_tstat(a, op, words, num_cus_current(), xcd_log2_current(), pp);
    if (rc) return rc;
  }
  if (query || *empty) return BLDP_OK;
  rc = check_banks("tstat: ", nbank, in);
  if (rc) return rc;
  if (!out) return fail(BLDP_EINVAL, "tstat: null output pointer");
  return check_out_strides("tstat: ", nbank, out_bank, out_ld_i, out_ld_b, a.nc, a.ni, a.nb);
}

static int tstat_run(int nbank, const float *const *in, int64_t nchan, int64_t nif, int64_t ntime,
                     const int64_t *win, int64_t tavby, int op, float *out, int64_t out_bank,
                     int64_t out_ld_i, int64_t out_ld_b, void *stream,
                     const double *qp = nullptr) {
  TStatArgs a;
  TStatPlan p;
  bool copy = false, empty = false;
  int rc = tstat_prepare(nbank, in, nchan, nif, ntime, win, tavby, op, out, out_bank, out_ld_i,
                         out_ld_b, false, &a, &p, &copy, &empty, qp);
  if (rc || empty) return rc;
  if (qp) op = kOpQuantile;
  hipStream_t s = (hipStream_t)stream;
  if (copy)  // the window itself: the reduce's F = T = 1 copy
    return reduce_impl(nbank, in, nchan, nif, ntime, win, 1, 1, BLDP_OP_SUM, out, out_bank,
                       out_ld_i, out_ld_b, false, s, nullptr);
  return run_planned("tstat", p.ws_bytes, s, [&](void *ws) {
    if (ws) a.ws = (double *)ws;
    return launch_tstat(a, p, op, s);
  });
}

int bldp_tstat_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int64_t tavby,
                     int64_t dims[3]) {
  return bldp_reduce_shape(nchan, nif, ntime, win, 1, tavby, dims);
}

// bldp_tstat_plan_f32, and with qp the time-axis plan of bldp_quantile_plan_f32
static int tstat_plan(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                      const int64_t *win, int64_t tavby, int op, const float *out,
                      int64_t info[8], const double *qp) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  TStatArgs a;
  TStatPlan p;
  bool copy = false, empty = false;
  const float *ins[1] = {in};
  int rc = tstat_prepare(1, ins, nchan, nif, ntime, win, tavby, op, (float *)out, 0, 0, 0, true,
                         &a, &p, &copy, &empty, qp);
  if (rc) return rc;
  if (copy) {  // the plan of the copy (bldp_reduce_plan_f32 of F = T = 1), path -1
    rc = bldp_reduce_plan_f32(in, nchan, nif, ntime, win, 1, 1, BLDP_OP_SUM, out, info);
    if (rc) return rc;
    const int64_t grid = info[5], ws = info[6];
    info[0] = -1, info[1] = 1, info[2] = 1, info[3] = 1, info[4] = grid, info[5] = ws;
    info[6] = a.nb, info[7] = 0;
    if (qp) info[5] = -1;  // (no rank: the window itself)
    return BLDP_OK;
  }
  fill_tstat_info(info, p, a);
  if (qp) info[5] = a.qrank;  // (no workspace: the slot carries the lower rank)
  return BLDP_OK;
}

int bldp_tstat_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                        const int64_t *win, int64_t tavby, int op, const float *out,
                        int64_t info[8]) {
  return tstat_plan(in, nchan, nif, ntime, win, tavby, op, out, info, nullptr);
}

int bldp_tstat_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                   int64_t tavby, int op, float *out, int64_t out_ld_i, int64_t out_ld_b,
                   void *stream) {
  const float *ins[1] = {in};
  return tstat_run(1, ins, nchan, nif, ntime, win, tavby, op, out, 0, out_ld_i, out_ld_b, stream);
}

int bldp_band_tstat_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                        int64_t ntime, const int64_t *win, int64_t tavby, int op, float *out,
                        void *stream) {
  int64_t l[4];
  const int rc = band_layout(nbank, nchan, nif, ntime, win, 1, tavby, l);
  if (rc) return rc;
  return tstat_run(nbank, in, nchan, nif, ntime, win, tavby, op, out, l[0], l[1], l[2], stream);
}

// ---- quantile(p): an order statistic of blocks of channels or of spectra -----
// The checks every bldp_quantile_* entry point makes before anything else.
static int quantile_check(int axis, double p) {
  if (axis != 0 && axis != 2)
    return fail(BLDP_EINVAL,
                "quantile: axis %d is not 0 (blocks of n channels) or 2 (blocks of n spectra)",
                axis);
  if (!(p >= 0.0 && p <= 1.0)) return fail(BLDP_EINVAL, "quantile: p=%g is outside [0, 1]", p);
  return BLDP_OK;
}

int bldp_quantile_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int axis,
                        int64_t n, int64_t dims[3]) {
  const int rc = quantile_check(axis, 0.0);
  if (rc) return rc;
  return bldp_reduce_shape(nchan, nif, ntime, win, axis == 0 ? n : 1, axis == 0 ? 1 : n, dims);
}

int bldp_quantile_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, int axis, int64_t n, double p, const float *out,
                           int64_t info[8]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  int rc = quantile_check(axis, p);
  if (rc) return rc;
  if (axis == 2) return tstat_plan(in, nchan, nif, ntime, win, n, 0, out, info, &p);
  int64_t sh[3];
  rc = bldp_reduce_shape(nchan, nif, ntime, win, n, 1, sh);
  if (rc) return rc;
  const float *ins[1] = {in};
  return reduce_impl(1, ins, nchan, nif, ntime, win, n, 1, 0, (float *)out, sh[0] * sh[1] * sh[2],
                     sh[0], sh[0] * sh[1], false, nullptr, info, &p);
}

int bldp_quantile_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                      const int64_t *win, int axis, int64_t n, double p, float *out,
                      int64_t out_ld_i, int64_t out_ld_t, void *stream) {
  const int rc = quantile_check(axis, p);
  if (rc) return rc;
  const float *ins[1] = {in};
  if (axis == 2)
    return tstat_run(1, ins, nchan, nif, ntime, win, n, 0, out, 0, out_ld_i, out_ld_t, stream, &p);
  return reduce_impl(1, ins, nchan, nif, ntime, win, n, 1, 0, out, 0, out_ld_i, out_ld_t, false,
                     (hipStream_t)stream, nullptr, &p);
}

int bldp_band_quantile_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                           int64_t ntime, const int64_t *win, int axis, int64_t n, double p,
                           float *out, void *stream) {
  int rc = quantile_check(axis, p);
  if (rc) return rc;
  if (axis == 0)
    return reduce_impl(nbank, in, nchan, nif, ntime, win, n, 1, 0, out, 0, 0, 0, true,
                       (hipStream_t)stream, nullptr, &p);
  int64_t l[4];  // (the vcat of the banks, as bldp_band_tstat_f32)
  rc = band_layout(nbank, nchan, nif, ntime, win, 1, n, l);
  if (rc) return rc;
  return tstat_run(nbank, in, nchan, nif, ntime, win, n, 0, out, l[0], l[1], l[2], stream, &p);
}

// ---- quantiles(ps): several quantiles of every block from one selection ------
// The checks every bldp_quantiles_* entry point makes before anything else.
static int quantiles_check(int axis, int np, const double *p) {
  int rc = quantile_check(axis, 0.0);
  if (rc) return rc;
  if (np < 1 || np > BLDP_MAX_QUANTILES)
    return fail(BLDP_EINVAL, "quantiles: np=%d outside 1..%d (batch longer lists)", np,
                BLDP_MAX_QUANTILES);
  if (!p) return fail(BLDP_EINVAL, "quantiles: null p");
  for (int k = 0; k < np; ++k)
    if (!(p[k] >= 0.0 && p[k] <= 1.0))
      return fail(BLDP_EINVAL, "quantiles: p[%d]=%g is outside [0, 1]", k, p[k]);
  return BLDP_OK;
}

// Every entry point of the family.  Plane k of the output starts at out + k *
// out_ld_q and is laid out as the quantile entry point of the same kind lays
// its one out (stitched: bldp_band_quantile_f32's dense product).  info: the
// plan query (nothing is launched).
static int quantiles_run(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int axis, int64_t n, int np,
                         const double *p, float *out, int64_t out_ld_i, int64_t out_ld_t,
                         int64_t out_ld_q, bool stitched, void *stream, int64_t *info) {
  int rc = quantiles_check(axis, np, p);
  if (rc) return rc;
  rc = check_nbank(nbank);
  if (rc) return rc;
  int64_t d[3];
  rc = bldp_quantile_shape(nchan, nif, ntime, win, axis, n, d);
  if (rc) return rc;
  int64_t bank = 0;
  if (stitched) {  // the vcat of the banks: dense planes one after the other
    vcat_layout(nbank, d, &bank, &out_ld_i, &out_ld_t);
    out_ld_q = out_ld_t * d[2];
  }
  const bool empty = d[0] == 0 || d[1] == 0 || d[2] == 0;
  if (!info && !empty && np > 1 &&
      out_ld_q < (d[2] - 1) * out_ld_t + (d[1] - 1) * out_ld_i + (stitched ? nbank : 1) * d[0])
    return fail(BLDP_EINVAL, "quantiles: planes %lld elements apart overlap for a (%lld, %lld, "
                "%lld) plane with strides (%lld, %lld)", (long long)out_ld_q, (long long)d[0],
                (long long)d[1], (long long)d[2], (long long)out_ld_i, (long long)out_ld_t);
  hipStream_t s = (hipStream_t)stream;
  if (n <= 1) {
    // the window itself in every plane, as the quantile entry point copies it
    if (info) {
      const float *ins[1] = {in ? in[0] : nullptr};
      if (axis == 2) {
        rc = tstat_plan(ins[0], nchan, nif, ntime, win, n, BLDP_OP_MEDIAN, nullptr, info, nullptr);
      } else {
        rc = reduce_impl(1, ins, nchan, nif, ntime, win, n, 1, BLDP_OP_MEDIAN, nullptr,
                         d[0] * d[1] * d[2], d[0], d[0] * d[1], false, nullptr, info);
      }
      info[8] = 0;
      info[9] = 1;
      return rc;
    }
    for (int k = 0; k < np && !rc; ++k) {
      float *o = out ? out + k * out_ld_q : nullptr;
      if (axis == 2)
        rc = tstat_run(nbank, in, nchan, nif, ntime, win, n, 0, o, bank, out_ld_i, out_ld_t,
                       stream, &p[k]);
      else
        rc = reduce_impl(nbank, in, nchan, nif, ntime, win, n, 1, 0, o, bank, out_ld_i, out_ld_t,
                         stitched, s, nullptr, &p[k]);
    }
    return rc;
  }
  QSet qs;
  quantile_set(n, np, p, out_ld_q, &qs);
  if (axis == 0) {
    RedArgs a;
    Plan pl;
    bool none = false;
    rc = prepare_reduce(nbank, in, nchan, nif, ntime, win, n, 1, 0, out, bank, out_ld_i, out_ld_t,
                        stitched, info != nullptr, &a, &pl, &none, nullptr, true);
    if (rc) return rc;
    if (info) {
      fill_reduce_info(info, pl, a);
      info[8] = qs.nr, info[9] = stats_q_reads(pl);
      return BLDP_OK;
    }
    if (none) return BLDP_OK;
    return run_planned("quantiles", 0, s, [&](void *) { return launch_stats_q(a, pl, qs, s); });
  }
  TStatArgs a;
  TStatPlan pl;
  bool copy = false, none = false;
  rc = tstat_prepare(nbank, in, nchan, nif, ntime, win, n, 0, out, bank, out_ld_i, out_ld_t,
                     info != nullptr, &a, &pl, &copy, &none, &p[0]);
  if (rc) return rc;
  bool words = true;
  for (int b = 0; b < nbank; ++b) words = words && aligned4(in[b]);
  rc = plan_tstat_q(a, qs.nlow, words, num_cus_current(), xcd_log2_current(), &pl);
  if (rc) return rc;
  if (info) {
    fill_tstat_info(info, pl, a);
    info[8] = qs.nr, info[9] = pl.passes;
    return BLDP_OK;
  }
  if (none) return BLDP_OK;
  return run_planned("quantiles", 0, s, [&](void *) { return launch_tstat_q(a, pl, qs, s); });
}

int bldp_quantiles_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int axis,
                         int64_t n, int np, int64_t dims[4]) {
  if (!dims) return fail(BLDP_EINVAL, "null dims");
  if (np < 1 || np > BLDP_MAX_QUANTILES)
    return fail(BLDP_EINVAL, "quantiles: np=%d outside 1..%d (batch longer lists)", np,
                BLDP_MAX_QUANTILES);
  const int rc = bldp_quantile_shape(nchan, nif, ntime, win, axis, n, dims);
  if (rc) return rc;
  dims[3] = np;
  return BLDP_OK;
}

int bldp_quantiles_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                            const int64_t *win, int axis, int64_t n, int np, const double *p,
                            const float *out, int64_t info[10]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  const float *ins[1] = {in};
  return quantiles_run(1, ins, nchan, nif, ntime, win, axis, n, np, p, (float *)out, 0, 0, 0,
                       true, nullptr, info);
}

int bldp_quantiles_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                       const int64_t *win, int axis, int64_t n, int np, const double *p,
                       float *out, int64_t out_ld_i, int64_t out_ld_t, int64_t out_ld_q,
                       void *stream) {
  const float *ins[1] = {in};
  return quantiles_run(1, ins, nchan, nif, ntime, win, axis, n, np, p, out, out_ld_i, out_ld_t,
                       out_ld_q, false, stream, nullptr);
}

int bldp_band_quantiles_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                            int64_t ntime, const int64_t *win, int axis, int64_t n, int np,
                            const double *p, float *out, void *stream) {
  return quantiles_run(nbank, in, nchan, nif, ntime, win, axis, n, np, p, out, 0, 0, 0, true,
                       stream, nullptr);
}

// ---- outliers: median, mad, count and flags of every block from one launch ----
// The checks every bldp_outliers_* entry point makes before anything else.
static int outliers_check(int axis, int64_t n, double nsigma) {
  if (axis != 0 && axis != 2)
    return fail(BLDP_EINVAL,
                "outliers: axis %d is not 0 (blocks of n channels) or 2 (blocks of n spectra)",
                axis);
  if (n < 2)
    return fail(BLDP_EINVAL, "outliers: n=%lld: a block of fewer than 2 values has no scale",
                (long long)n);
  if (!(nsigma >= 0.0) || std::isinf(nsigma))
    return fail(BLDP_EINVAL, "outliers: nsigma=%g is not a finite number >= 0", nsigma);
  return BLDP_OK;
}

int bldp_outliers_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int axis,
                        int64_t n, int64_t dims[3], int64_t mask_dims[3]) {
  if (!dims || !mask_dims) return fail(BLDP_EINVAL, "null dims");
  int rc = outliers_check(axis, n, 0.0);
  if (rc) return rc;
  rc = bldp_quantile_shape(nchan, nif, ntime, win, axis, n, dims);
  if (rc) return rc;
  mask_dims[0] = axis == 0 ? dims[0] * n : dims[0];
  mask_dims[1] = dims[1];
  mask_dims[2] = axis == 2 ? dims[2] * n : dims[2];
  return BLDP_OK;
}

// Every entry point of the family.  med, mad and count: element (c', i, t') of
// bank b at [b*bank + c' + i*out_ld_i + t'*out_ld_t] (stitched: the dense vcat
// of the banks, as bldp_band_quantile_f32's product; the mask is then the vcat
// of the banks' windows).  info: the plan query (nothing is launched).
static int outliers_run(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                        int64_t ntime, const int64_t *win, int axis, int64_t n, double nsigma,
                        float *med, float *mad, uint32_t *count, uint8_t *mask, int64_t out_ld_i,
                        int64_t out_ld_t, bool stitched, void *stream, int64_t *info,
                        bool want_mask) {
  int rc = outliers_check(axis, n, nsigma);
  if (rc) return rc;
  rc = check_nbank(nbank);
  if (rc) return rc;
  int64_t d[3], md[3];
  rc = bldp_outliers_shape(nchan, nif, ntime, win, axis, n, d, md);
  if (rc) return rc;
  int64_t bank = 0;
  if (stitched) vcat_layout(nbank, d, &bank, &out_ld_i, &out_ld_t);
  const bool empty = d[0] == 0 || d[1] == 0 || d[2] == 0;
  if (!info && !empty) {
    if (!in) return fail(BLDP_EINVAL, "outliers: null input pointer array");
    rc = check_banks("outliers: ", nbank, in);
    if (rc) return rc;
    if (!med && !mad && !count && !mask)
      return fail(BLDP_EINVAL, "outliers: every output is null");
    if (med || mad || count) {
      rc = check_out_strides("outliers: ", 1, 0, out_ld_i, out_ld_t, d[0], d[1], d[2]);
      if (rc) return rc;
    }
    // the outputs may not overlap each other or the input arrays (the whole
    // arrays, where the later families check the window's span)
    const int64_t span =
        (nbank - 1) * bank + (d[2] - 1) * out_ld_t + (d[1] - 1) * out_ld_i + d[0];
    const void *ptr[4] = {med, mad, count, mask};
    const size_t len[4] = {(size_t)span * 4, (size_t)span * 4, (size_t)span * 4,
                           (size_t)(nbank * md[0] * md[1] * md[2])};
    static const char *const name[4] = {"med", "mad", "count", "mask"};
    for (int q = 0; q < 4; ++q) {
      if (!ptr[q]) continue;
      for (int r = q + 1; r < 4; ++r)
        if (ptr[r] && spans_overlap(ptr[q], len[q], ptr[r], len[r]))
          return fail(BLDP_EINVAL, "outliers: outputs %s and %s overlap", name[q], name[r]);
      for (int b = 0; b < nbank; ++b)
        if (spans_overlap(ptr[q], len[q], in[b], (size_t)(nchan * nif * ntime) * sizeof(float)))
          return fail(BLDP_EINVAL, "outliers: output %s overlaps the input (bank %d)", name[q], b);
    }
  }
  OutlArgs oa{};
  oa.nsigma = std::fabs(nsigma);  // (-0.0: the threshold's key must be +0.0's)
  oa.med = med, oa.mad = mad, oa.count = count, oa.mask = mask;
  oa.mask_bank = stitched ? md[0] : 0;
  oa.mask_ld_i = nbank * md[0];
  oa.mask_ld_t = oa.mask_ld_i * md[1];
  const bool wm = info ? want_mask : mask != nullptr;
  const float *none_in[BLDP_MAX_BANKS] = {};
  if (!in) in = none_in;  // (the plan query takes null pointers)
  hipStream_t s = (hipStream_t)stream;
  if (axis == 0) {
    RedArgs a;
    Plan pl;
    bool none = false;
    rc = prepare_reduce(nbank, in, nchan, nif, ntime, win, n, 1, BLDP_OP_MAD, nullptr, bank,
                        out_ld_i, out_ld_t, false, true, &a, &pl, &none);
    if (rc) return rc;
    if (info) {
      fill_reduce_info(info, pl, a);
      info[8] = stats_outl_reads(pl, wm), info[9] = wm ? 1 : 0;
      return BLDP_OK;
    }
    if (none) return BLDP_OK;
    return run_planned("outliers", 0, s, [&](void *) { return launch_stats_outl(a, pl, oa, s); });
  }
  TStatArgs a;
  TStatPlan pl;
  bool copy = false, none = false;
  rc = tstat_prepare(nbank, in, nchan, nif, ntime, win, n, BLDP_OP_MAD, nullptr, bank, out_ld_i,
                     out_ld_t, true, &a, &pl, &copy, &none);
  if (rc) return rc;
  if (info) {
    fill_tstat_info(info, pl, a);
    info[8] = tstat_outl_reads(pl, wm), info[9] = wm ? 1 : 0;
    return BLDP_OK;
  }
  if (none) return BLDP_OK;
  return run_planned("outliers", 0, s, [&](void *) { return launch_tstat_outl(a, pl, oa, s); });
}

int bldp_outliers_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, int axis, int64_t n, int want_mask,
                           int64_t info[10]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  const float *ins[1] = {in};
  return outliers_run(1, ins, nchan, nif, ntime, win, axis, n, 0.0, nullptr, nullptr, nullptr,
                      nullptr, 0, 0, true, nullptr, info, want_mask != 0);
}

int bldp_outliers_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                      const int64_t *win, int axis, int64_t n, double nsigma, float *med,
                      float *mad, uint32_t *count, uint8_t *mask, int64_t out_ld_i,
                      int64_t out_ld_t, void *stream) {
  const float *ins[1] = {in};
  return outliers_run(1, ins, nchan, nif, ntime, win, axis, n, nsigma, med, mad, count, mask,
                      out_ld_i, out_ld_t, false, stream, nullptr, false);
}

int bldp_band_outliers_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                           int64_t ntime, const int64_t *win, int axis, int64_t n, double nsigma,
                           float *med, float *mad, uint32_t *count, uint8_t *mask, void *stream) {
  return outliers_run(nbank, in, nchan, nif, ntime, win, axis, n, nsigma, med, mad, count, mask,
                      0, 0, true, stream, nullptr, false);
}

// ---- fqavfunc argmax / argmin: the winner's offset in every F x T block ------
// Checks, window and plan of an argext (every entry point).  The outputs'
// element (c', i, t') of bank b sits at [b*out_bank + c' + i*out_ld_i + t'*out_ld_t].
static int argext_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                          int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                          int argop, uint32_t *idx, float *val, int64_t out_bank,
                          int64_t out_ld_i, int64_t out_ld_t, bool query, ArgArgs *ap, Plan *pp,
                          bool *empty) {
  static const char what[] = "argext: ";
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (argop != BLDP_ARG_MAX && argop != BLDP_ARG_MIN)
    return fail(BLDP_EINVAL, "argext: unknown argop %d (0=argmax 1=argmin)", argop);
  Geo g;
  int64_t F, T;
  rc = resolve_blocks(nchan, nif, ntime, win, fqavby, tavby, &g, &F, &T);
  if (!rc) rc = check_block31(what, F, T);  // (the offsets)
  if (rc) return rc;
  ArgArgs &aa = *ap;
  aa = ArgArgs{};
  RedArgs &a = aa.r;
  *empty = set_blocks(a, g, F, T, out_bank, out_ld_i, out_ld_t);
  a.out = val;
  aa.idx = idx;
  aa.inv = argop == BLDP_ARG_MIN ? 0xffffffffu : 0u;
  bool words;
  rc = set_window(what, a, g, nbank, in, &words);
  if (!rc) rc = plan_argext(aa, words && g.cs == 1, num_cus_current(), xcd_log2_current(), pp);
  if (rc || query || *empty) return rc;
  rc = check_banks(what, nbank, in);
  if (rc) return rc;
  if (!idx) return fail(BLDP_EINVAL, "argext: null idx pointer");
  rc = check_out_strides(what, nbank, out_bank, out_ld_i, out_ld_t, a.nco, a.ni, a.nto);
  if (rc) return rc;
  // the outputs may not overlap the window's elements (one message for both),
  // nor each other
  int64_t lo;
  size_t wbytes;
  window_span(g, &lo, &wbytes);
  const size_t obytes = 4 * (size_t)((nbank - 1) * out_bank + (a.nco - 1) +
                                     (a.ni - 1) * out_ld_i + (a.nto - 1) * out_ld_t + 1);
  for (int b = 0; b < nbank; ++b)
    if (spans_overlap(idx, obytes, in[b] + lo, wbytes) ||
        (val && spans_overlap(val, obytes, in[b] + lo, wbytes)))
      return fail(BLDP_EINVAL, "argext: idx / val overlap the input window (bank %d)", b);
  if (val && spans_overlap(idx, obytes, val, obytes))
    return fail(BLDP_EINVAL, "argext: idx and val overlap");
  return BLDP_OK;
}

static int argext_run(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                      int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby, int argop,
                      uint32_t *idx, float *val, int64_t out_bank, int64_t out_ld_i,
                      int64_t out_ld_t, void *stream) {
  ArgArgs a;
  Plan p;
  bool empty = false;
  int rc = argext_prepare(nbank, in, nchan, nif, ntime, win, fqavby, tavby, argop, idx, val,
                          out_bank, out_ld_i, out_ld_t, false, &a, &p, &empty);
  if (rc || empty) return rc;
  hipStream_t s = (hipStream_t)stream;
  return run_planned("argext", 0, s, [&](void *) { return launch_argext(a, p, s); });
}

int bldp_argext_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                         const int64_t *win, int64_t fqavby, int64_t tavby, int argop,
                         const uint32_t *idx, int64_t info[8]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  ArgArgs a;
  Plan p;
  bool empty = false;
  const float *ins[1] = {in};
  int rc = argext_prepare(1, ins, nchan, nif, ntime, win, fqavby, tavby, argop, (uint32_t *)idx,
                          nullptr, 0, 0, 0, true, &a, &p, &empty);
  if (rc) return rc;
  info[0] = p.path;
  info[1] = p.lpg;
  info[2] = a.r.ts;
  info[3] = a.r.k4;
  info[4] = p.grid;
  info[5] = (int64_t)p.ws_bytes;
  info[6] = p.nout;
  info[7] = a.r.k4 != 0;
  return BLDP_OK;
}

int bldp_argext_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, int64_t fqavby, int64_t tavby, int argop, uint32_t *idx,
                    float *val, int64_t out_ld_i, int64_t out_ld_t, void *stream) {
  const float *ins[1] = {in};
  return argext_run(1, ins, nchan, nif, ntime, win, fqavby, tavby, argop, idx, val, 0, out_ld_i,
                    out_ld_t, stream);
}

int bldp_band_argext_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                         int argop, uint32_t *idx, float *val, void *stream) {
  int64_t l[4];
  const int rc = band_layout(nbank, nchan, nif, ntime, win, fqavby, tavby, l);
  if (rc) return rc;
  return argext_run(nbank, in, nchan, nif, ntime, win, fqavby, tavby, argop, idx, val, l[0],
                    l[1], l[2], stream);
}

// ---- masked reduce: the sum / mean of a block's unflagged samples and their count ----
// Checks, window and plan of a masked reduce (every entry point).  The outputs'
// element (c', i, t') of bank b sits at [b*out_bank + c' + i*out_ld_i + t'*out_ld_t];
// bank b's channel c is channel b*nc + c of the mask.  mask_ld NULL: the dense
// (nbank*nc, ni, nt) mask.  query: the plan call (null pointers count as aligned).
static int masked_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                          int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                          int op, const uint8_t *mask, const int64_t *mask_ld, float *out,
                          uint32_t *kept, int64_t out_bank, int64_t out_ld_i, int64_t out_ld_t,
                          bool query, MaskedArgs *ap, Plan *pp, bool *empty) {
  static const char what[] = "masked reduce: ";
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (op != BLDP_OP_SUM && op != BLDP_OP_MEAN)
    return fail(BLDP_EINVAL, "masked reduce: op %d is not sum (%d) or mean (%d)", op, BLDP_OP_SUM,
                BLDP_OP_MEAN);
  Geo g;
  int64_t F, T, ld[3];
  rc = resolve_blocks(nchan, nif, ntime, win, fqavby, tavby, &g, &F, &T);
  if (!rc) rc = check_block31(what, F, T);  // (kept)
  if (!rc) rc = mask_strides(what, mask_ld, nbank * g.nc, g.ni, ld);
  if (rc) return rc;
  MaskedArgs &ma = *ap;
  ma = MaskedArgs{};
  RedArgs &a = ma.r;
  *empty = set_blocks(a, g, F, T, out_bank, out_ld_i, out_ld_t);
  a.out = out;
  ma.kept = kept;
  ma.mask = mask;
  ma.m_cs = ld[0], ma.m_ld_i = ld[1], ma.m_ld_t = ld[2];
  ma.m_bank = g.nc * ld[0];
  ma.mean = op == BLDP_OP_MEAN;
  bool words;
  rc = set_window(what, a, g, nbank, in, &words);
  if (!rc)
    rc = plan_masked(ma, words && g.cs == 1, aligned4(mask), num_cus_current(),
                     xcd_log2_current(), pp);
  if (rc || query || *empty) return rc;
  rc = check_banks(what, nbank, in);
  if (rc) return rc;
  if (!out && !kept) return fail(BLDP_EINVAL, "masked reduce: out and kept are both null");
  if (!mask) return fail(BLDP_EINVAL, "masked reduce: null mask pointer");
  rc = check_out_strides(what, nbank, out_bank, out_ld_i, out_ld_t, a.nco, a.ni, a.nto);
  if (rc) return rc;
  const size_t obytes = 4 * (size_t)((nbank - 1) * out_bank + (a.nco - 1) +
                                     (a.ni - 1) * out_ld_i + (a.nto - 1) * out_ld_t + 1);
  const Span outs[2] = {{out, obytes, "out"}, {kept, obytes, "kept"}};
  return check_disjoint(what, outs, 2, g, nbank, in,
                        {mask, mask_span_bytes(nbank * g.nc, g.ni, g.nt, ld), "the mask"});
}

static int masked_run(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                      int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby, int op,
                      const uint8_t *mask, const int64_t *mask_ld, float *out, uint32_t *kept,
                      int64_t out_bank, int64_t out_ld_i, int64_t out_ld_t, void *stream) {
  MaskedArgs a;
  Plan p;
  bool empty = false;
  int rc = masked_prepare(nbank, in, nchan, nif, ntime, win, fqavby, tavby, op, mask, mask_ld, out,
                          kept, out_bank, out_ld_i, out_ld_t, false, &a, &p, &empty);
  if (rc || empty) return rc;
  hipStream_t s = (hipStream_t)stream;
  return run_planned("masked reduce", 0, s, [&](void *) { return launch_masked(a, p, s); });
}

int bldp_masked_reduce_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                const int64_t *win, int64_t fqavby, int64_t tavby,
                                const uint8_t *mask, const int64_t *mask_ld, int64_t info[10]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  MaskedArgs a;
  Plan p;
  bool empty = false;
  const float *ins[1] = {in};
  int rc = masked_prepare(1, ins, nchan, nif, ntime, win, fqavby, tavby, BLDP_OP_SUM, mask,
                          mask_ld, nullptr, nullptr, 0, 0, 0, true, &a, &p, &empty);
  if (rc) return rc;
  info[0] = p.path;
  info[1] = p.lpg;
  info[2] = a.r.ts;
  info[3] = a.r.k4;
  info[4] = p.grid;
  info[5] = (int64_t)p.ws_bytes;
  info[6] = p.nout;
  info[7] = a.r.k4 != 0;
  info[8] = a.mform;
  info[9] = 0;
  return BLDP_OK;
}

int bldp_masked_reduce_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, int64_t fqavby, int64_t tavby, int op,
                           const uint8_t *mask, const int64_t *mask_ld, float *out,
                           uint32_t *kept, int64_t out_ld_i, int64_t out_ld_t, void *stream) {
  const float *ins[1] = {in};
  return masked_run(1, ins, nchan, nif, ntime, win, fqavby, tavby, op, mask, mask_ld, out, kept,
                    0, out_ld_i, out_ld_t, stream);
}

int bldp_band_masked_reduce_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                int64_t ntime, const int64_t *win, int64_t fqavby,
                                int64_t tavby, int op, const uint8_t *mask,
                                const int64_t *mask_ld, float *out, uint32_t *kept,
                                void *stream) {
  int64_t l[4];
  const int rc = band_layout(nbank, nchan, nif, ntime, win, fqavby, tavby, l);
  if (rc) return rc;
  return masked_run(nbank, in, nchan, nif, ntime, win, fqavby, tavby, op, mask, mask_ld, out,
                    kept, l[0], l[1], l[2], stream);
}

// ---- histogram: the counts per bin of every block, with below / above / nan ----
// Checks, window and plan of a histogram (every entry point).  Plane q of block
// (c', i, t') of bank b sits at [b*out_bank + c' + i*out_ld_i + t'*out_ld_t +
// q*out_ld_q].  query: the plan call (null pointers count as aligned).
static int hist_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                        int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                        int nbins, double lo, double hi, uint32_t *out, int64_t out_bank,
                        int64_t out_ld_i, int64_t out_ld_t, int64_t out_ld_q, bool query,
                        HistArgs *ap, Plan *pp, bool *empty) {
  static const char what[] = "histogram: ";
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (nbins < 1 || nbins > BLDP_MAX_HIST_BINS)
    return fail(BLDP_EINVAL, "histogram: nbins=%d outside 1..%d", nbins, BLDP_MAX_HIST_BINS);
  const float lo32 = (float)lo, hi32 = (float)hi;
  if (!std::isfinite(lo32) || !std::isfinite(hi32) || !(lo32 < hi32))
    return fail(BLDP_EINVAL, "histogram: Float32(lo)=%g and Float32(hi)=%g must be finite with "
                "lo < hi", (double)lo32, (double)hi32);
  const volatile float w = hi32 - lo32;  // (one Float32 operation each, as written)
  if (!std::isfinite(w))
    return fail(BLDP_EINVAL, "histogram: hi - lo overflows Float32 (lo=%g, hi=%g)", (double)lo32,
                (double)hi32);
  const volatile float sc = (float)nbins / w;
  if (!std::isfinite(sc) || !(sc > 0.0f))
    return fail(BLDP_EINVAL, "histogram: the bin scale nbins / (hi - lo) = %g is not a finite "
                "positive Float32 (nbins=%d, lo=%g, hi=%g)", (double)sc, nbins, (double)lo32,
                (double)hi32);
  Geo g;
  int64_t F, T;
  rc = resolve_blocks(nchan, nif, ntime, win, fqavby, tavby, &g, &F, &T);
  if (!rc) rc = check_block31(what, F, T);  // (the counts)
  if (rc) return rc;
  HistArgs &a = *ap;
  a = HistArgs{};
  *empty = set_blocks(a, g, F, T, out_bank, out_ld_i, out_ld_t);
  a.B = nbins;
  a.lo = lo32, a.hi = hi32, a.s = sc;
  a.out = out;
  a.out_ld_q = out_ld_q;
  bool words;
  rc = set_window(what, a, g, nbank, in, &words);
  if (!rc) rc = plan_hist(a, words && g.cs == 1, num_cus_current(), pp);
  if (rc || query || *empty) return rc;
  rc = check_banks(what, nbank, in);
  if (rc) return rc;
  if (!out) return fail(BLDP_EINVAL, "histogram: null output pointer");
  const int64_t plane = (nbank - 1) * out_bank + (a.nco - 1) + (a.ni - 1) * out_ld_i +
                        (a.nto - 1) * out_ld_t + 1;  // the extent of a plane
  if (out_ld_i < a.nco || out_ld_t < (a.ni - 1) * out_ld_i + a.nco ||
      (nbank > 1 && out_bank < a.nco) || out_ld_q < plane)
    return fail(BLDP_EINVAL, "histogram: out strides (%lld, %lld, %lld) overlap for a (%lld, %lld, "
                "%lld, %d) result", (long long)out_ld_i, (long long)out_ld_t, (long long)out_ld_q,
                (long long)a.nco, (long long)a.ni, (long long)a.nto, nbins + 3);
  const Span outs[1] = {{out, 4 * (size_t)((int64_t)(nbins + 2) * out_ld_q + plane), "out"}};
  return check_disjoint(what, outs, 1, g, nbank, in, {nullptr, 0, ""});
}

static int hist_run(int nbank, const float *const *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, int64_t fqavby, int64_t tavby, int nbins, double lo,
                    double hi, uint32_t *out, int64_t out_bank, int64_t out_ld_i,
                    int64_t out_ld_t, int64_t out_ld_q, void *stream) {
  HistArgs a;
  Plan p;
  bool empty = false;
  int rc = hist_prepare(nbank, in, nchan, nif, ntime, win, fqavby, tavby, nbins, lo, hi, out,
                        out_bank, out_ld_i, out_ld_t, out_ld_q, false, &a, &p, &empty);
  if (rc || empty) return rc;
  hipStream_t s = (hipStream_t)stream;
  return run_planned("histogram", 0, s, [&](void *) { return launch_hist(a, p, s); });
}

int bldp_histogram_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                            const int64_t *win, int64_t fqavby, int64_t tavby, int nbins,
                            double lo, double hi, int64_t info[10]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  HistArgs a;
  Plan p;
  bool empty = false;
  const float *ins[1] = {in};
  int rc = hist_prepare(1, ins, nchan, nif, ntime, win, fqavby, tavby, nbins, lo, hi, nullptr, 0,
                        0, 0, 0, true, &a, &p, &empty);
  if (rc) return rc;
  info[0] = p.path;
  info[1] = p.grid;
  info[2] = (int64_t)a.nchunk * a.ctiles;
  info[3] = a.G;
  info[4] = p.shm;
  info[5] = a.R;
  info[6] = (int64_t)p.ws_bytes;
  info[7] = a.vec != 0;
  info[8] = p.lpg;
  info[9] = a.rows_per_chunk;
  return BLDP_OK;
}

int bldp_histogram_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                       const int64_t *win, int64_t fqavby, int64_t tavby, int nbins, double lo,
                       double hi, uint32_t *out, int64_t out_ld_i, int64_t out_ld_t,
                       int64_t out_ld_q, void *stream) {
  const float *ins[1] = {in};
  return hist_run(1, ins, nchan, nif, ntime, win, fqavby, tavby, nbins, lo, hi, out, 0, out_ld_i,
                  out_ld_t, out_ld_q, stream);
}

int bldp_band_histogram_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                            int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                            int nbins, double lo, double hi, uint32_t *out, void *stream) {
  int64_t l[4];  // (the vcat of every plane)
  const int rc = band_layout(nbank, nchan, nif, ntime, win, fqavby, tavby, l);
  if (rc) return rc;
  return hist_run(nbank, in, nchan, nif, ntime, win, fqavby, tavby, nbins, lo, hi, out, l[0],
                  l[1], l[2], l[3], stream);
}

// ---- hits: the flagged samples of a window as an ordered list ----
// Checks, window and plan of a hits call (every entry point).  The window is
// the vcat (nbank*nc, ni, nt) of the banks; mask_ld NULL: the dense mask of that
// shape.  query: the plan call (null pointers count as aligned).
static int hits_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                        int64_t ntime, const int64_t *win, const uint8_t *mask,
                        const int64_t *mask_ld, int64_t cap, int64_t *idx, float *val,
                        uint64_t *total, bool query, HitsArgs *ap, Plan *pp, bool *empty) {
  static const char what[] = "hits: ";
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (cap < 0) return fail(BLDP_EINVAL, "hits: cap=%lld is negative", (long long)cap);
  if (!query && !total) return fail(BLDP_EINVAL, "hits: null total pointer");
  Geo g;
  rc = resolve_window(nchan, nif, ntime, win, &g);
  if (rc) return rc;
  const int64_t NC = nbank * g.nc;
  int64_t ld[3];
  rc = mask_strides(what, mask_ld, NC, g.ni, ld);
  if (rc) return rc;
  HitsArgs &a = *ap;
  a = HitsArgs{};
  a.nc = g.nc, a.NC = NC, a.ni = g.ni, a.nt = g.nt;
  a.N = NC * g.ni * g.nt;
  a.mask = mask;
  a.m_cs = ld[0], a.m_ld_i = ld[1], a.m_ld_t = ld[2];
  a.cap = cap;
  a.idx = idx;
  a.val = reinterpret_cast<uint32_t *>(val);
  a.total = total;
  *empty = a.N == 0;
  *pp = Plan{};
  if (*empty) return BLDP_OK;
  rc = set_window(what, a, g, nbank, in);
  if (!rc) rc = plan_hits(a, (uintptr_t)mask, pp);
  if (rc || query) return rc;
  rc = check_banks(what, nbank, in);
  if (rc) return rc;
  if (!mask) return fail(BLDP_EINVAL, "hits: null mask pointer");
  const size_t n = (size_t)std::min(cap, a.N);  // entries a list can get
  const Span outs[3] = {{idx, 8 * n, "idx"}, {val, 4 * n, "val"}, {total, 8, "total"}};
  return check_disjoint(what, outs, 3, g, nbank, in,
                        {mask, mask_span_bytes(NC, g.ni, g.nt, ld), "the mask"});
}

static int hits_run(int nbank, const float *const *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, const uint8_t *mask, const int64_t *mask_ld, int64_t cap,
                    int64_t *idx, float *val, uint64_t *total, void *stream) {
  HitsArgs a;
  Plan p;
  bool empty = false;
  int rc = hits_prepare(nbank, in, nchan, nif, ntime, win, mask, mask_ld, cap, idx, val, total,
                        false, &a, &p, &empty);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (empty) {  // no launch: total = 0
    HIPCHK(hipMemsetAsync(total, 0, sizeof(uint64_t), s));
    return BLDP_OK;
  }
  return run_planned("hits", p.ws_bytes, s, [&](void *ws) {  // (never 0: 12 bytes a tile)
    a.woff = static_cast<uint64_t *>(ws);
    a.wcount = reinterpret_cast<uint32_t *>(a.woff + a.tiles);
    return launch_hits(a, p, cap > 0 && (idx || val), s);
  });
}

int bldp_hits_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                       const int64_t *win, const uint8_t *mask, const int64_t *mask_ld,
                       int64_t cap, int64_t info[10]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  HitsArgs a;
  Plan p;
  bool empty = false;
  const float *ins[1] = {in};
  int rc = hits_prepare(1, ins, nchan, nif, ntime, win, mask, mask_ld, cap, nullptr, nullptr,
                        nullptr, true, &a, &p, &empty);
  if (rc) return rc;
  for (int q = 0; q < 10; ++q) info[q] = 0;
  if (empty) return BLDP_OK;  // (nothing is launched)
  info[0] = p.path;
  info[1] = a.E;
  info[2] = a.tiles;
  info[3] = (int64_t)p.ws_bytes;
  info[4] = p.nout;
  info[5] = a.W;
  info[6] = cap == 0 ? 2 : 3;
  return BLDP_OK;
}

int bldp_hits_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                  const uint8_t *mask, const int64_t *mask_ld, int64_t cap, int64_t *idx,
                  float *val, uint64_t *total, void *stream) {
  const float *ins[1] = {in};
  return hits_run(1, ins, nchan, nif, ntime, win, mask, mask_ld, cap, idx, val, total, stream);
}

int bldp_band_hits_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                       int64_t ntime, const int64_t *win, const uint8_t *mask,
                       const int64_t *mask_ld, int64_t cap, int64_t *idx, float *val,
                       uint64_t *total, void *stream) {
  return hits_run(nbank, in, nchan, nif, ntime, win, mask, mask_ld, cap, idx, val, total, stream);
}

// ---- fold / unfold: a window over its coarse channels, and back ----
// The window, nfpc and T of a fold or an unfold: J = nc / nfpc coarse channels per
// bank, nto = nt / T time blocks.
static int fold_geometry(int nbank, int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                         int64_t nfpc, int64_t tavby, Geo *g, int64_t *J, int64_t *T) {
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (nfpc < 1) return fail(BLDP_EINVAL, "fold: nfpc=%lld is less than 1", (long long)nfpc);
  rc = resolve_window(nchan, nif, ntime, win, g);
  if (rc) return rc;
  *T = tavby <= 1 ? 1 : tavby;
  if (g->nc % nfpc != 0)
    return fail(BLDP_EDIM, "DimensionMismatch: nfpc=%lld does not divide nchan=%lld",
                (long long)nfpc, (long long)g->nc);
  if (g->nt % *T != 0)
    return fail(BLDP_EDIM, "DimensionMismatch: tavby=%lld does not divide ntime=%lld",
                (long long)*T, (long long)g->nt);
  *J = g->nc / nfpc;
  return BLDP_OK;
}

// 16-byte loads of every float4 of a unit-step window's rows are legal
static bool fold_vec_ok(int nbank, const float *const *in, const Geo &g) {
  if (g.cs != 1 || g.off % 4 != 0) return false;
  if ((g.ni > 1 && g.ld_i % 4 != 0) || (g.nt > 1 && g.ld_t % 4 != 0)) return false;
  for (int b = 0; b < nbank; ++b)
    if (!aligned16(in[b])) return false;
  return true;
}

// Checks, window and plan of a fold (every entry point).  has_mask: the plan call
// asks with a null mask pointer, which counts as aligned.
static int fold_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                        int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby, int op,
                        const uint8_t *mask, bool has_mask, const int64_t *mask_ld, float *out,
                        uint32_t *kept, int64_t out_ld_i, int64_t out_ld_t, bool query,
                        FoldArgs *ap, Plan *pp, bool *empty) {
  static const char what[] = "fold: ";
  Geo g;
  int64_t J, T;
  int rc = fold_geometry(nbank, nchan, nif, ntime, win, nfpc, tavby, &g, &J, &T);
  if (rc) return rc;
  if (op != BLDP_OP_SUM && op != BLDP_OP_MEAN)
    return fail(BLDP_EINVAL, "fold: op %d is not sum (%d) or mean (%d)", op, BLDP_OP_SUM,
                BLDP_OP_MEAN);
  // kept is 31-bit (Python and the shim read Int32)
  if (nbank * J > INT32_MAX / T)
    return fail(BLDP_EINVAL, "fold: blocks of J x tavby = %lld x %lld samples are beyond 2^31 - 1",
                (long long)(nbank * J), (long long)T);
  int64_t ld[3] = {0, 0, 0};
  if (has_mask) {
    rc = mask_strides(what, mask_ld, nbank * g.nc, g.ni, ld);
    if (rc) return rc;
  }
  FoldArgs &a = *ap;
  a = FoldArgs{};
  a.out = out, a.kept = kept, a.mask = mask;
  a.m_cs = ld[0], a.m_ld_i = ld[1], a.m_ld_t = ld[2], a.m_bank = g.nc * ld[0];
  a.out_ld_i = out_ld_i, a.out_ld_t = out_ld_t;
  a.nfpc = nfpc, a.J = J, a.ni = g.ni, a.T = T, a.nto = g.nt / T;
  a.mean = op == BLDP_OP_MEAN;
  a.mask_present = has_mask;
  *empty = g.nc == 0 || g.ni == 0 || g.nt == 0;
  rc = set_window(what, a, g, nbank, in);
  if (!rc) rc = plan_fold(a, fold_vec_ok(nbank, in, g), aligned4(mask), num_cus_current(), pp);
  if (rc || query || *empty) return rc;
  rc = check_banks(what, nbank, in);
  if (rc) return rc;
  if (!out && !kept) return fail(BLDP_EINVAL, "fold: out and kept are both null");
  rc = check_out_strides(what, 1, 0, out_ld_i, out_ld_t, nfpc, g.ni, a.nto);
  if (rc) return rc;
  const size_t obytes =
      4 * (size_t)((nfpc - 1) + (g.ni - 1) * out_ld_i + (a.nto - 1) * out_ld_t + 1);
  const Span outs[2] = {{out, obytes, "out"}, {kept, obytes, "kept"}};
  return check_disjoint(
      what, outs, 2, g, nbank, in,
      {mask, has_mask ? mask_span_bytes(nbank * g.nc, g.ni, g.nt, ld) : 0, "the mask"});
}

static int fold_run(int nbank, const float *const *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, int64_t nfpc, int64_t tavby, int op, const uint8_t *mask,
                    const int64_t *mask_ld, float *out, uint32_t *kept, int64_t out_ld_i,
                    int64_t out_ld_t, void *stream) {
  FoldArgs a;
  Plan p;
  bool empty = false;
  int rc = fold_prepare(nbank, in, nchan, nif, ntime, win, nfpc, tavby, op, mask, mask != nullptr,
                        mask_ld, out, kept, out_ld_i, out_ld_t, false, &a, &p, &empty);
  if (rc || empty) return rc;
  hipStream_t s = (hipStream_t)stream;
  return run_planned("fold", p.ws_bytes, s, [&](void *ws) {
    if (ws) {  // the chunks' partials, held until the merge is queued
      a.ws_sum = static_cast<double *>(ws);
      a.ws_kept = reinterpret_cast<uint32_t *>(a.ws_sum + (size_t)a.nchunk * (size_t)a.nout);
    }
    return launch_fold(a, p, s);
  });
}

int bldp_fold_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int64_t nfpc,
                    int64_t tavby, int64_t out_shape[3]) {
  if (!out_shape) return fail(BLDP_EINVAL, "null out_shape");
  Geo g;
  int64_t J, T;
  int rc = fold_geometry(1, nchan, nif, ntime, win, nfpc, tavby, &g, &J, &T);
  if (rc) return rc;
  out_shape[0] = g.nc == 0 ? 0 : nfpc;
  out_shape[1] = g.ni;
  out_shape[2] = g.nt / T;
  return BLDP_OK;
}

int bldp_fold_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                       const int64_t *win, int64_t nfpc, int64_t tavby, const uint8_t *mask,
                       const int64_t *mask_ld, int64_t info[10]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  FoldArgs a;
  Plan p;
  bool empty = false;
  const float *ins[1] = {in};
  int rc = fold_prepare(1, ins, nchan, nif, ntime, win, nfpc, tavby, BLDP_OP_SUM, mask,
                        mask != nullptr || mask_ld != nullptr, mask_ld, nullptr, nullptr, 0, 0,
                        true, &a, &p, &empty);
  if (rc) return rc;
  for (int q = 0; q < 10; ++q) info[q] = 0;
  if (empty) return BLDP_OK;  // (nothing is launched)
  info[0] = p.path;
  info[1] = p.lpg;
  info[2] = a.nchunk;
  info[3] = p.grid;
  info[4] = (int64_t)p.ws_bytes;
  info[5] = a.nchunk > 1 ? 2 : 1;
  info[6] = a.mform;
  info[7] = a.vec;
  info[8] = a.nout;
  info[9] = a.CU;
  return BLDP_OK;
}

int bldp_fold_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                  int64_t nfpc, int64_t tavby, int op, const uint8_t *mask,
                  const int64_t *mask_ld, float *out, uint32_t *kept, int64_t out_ld_i,
                  int64_t out_ld_t, void *stream) {
  const float *ins[1] = {in};
  return fold_run(1, ins, nchan, nif, ntime, win, nfpc, tavby, op, mask, mask_ld, out, kept,
                  out_ld_i, out_ld_t, stream);
}

int bldp_band_fold_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                       int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby, int op,
                       const uint8_t *mask, const int64_t *mask_ld, float *out, uint32_t *kept,
                       void *stream) {
  int64_t d[3];
  int rc = bldp_fold_shape(nchan, nif, ntime, win, nfpc, tavby, d);
  if (rc) return rc;
  // ONE dense (nfpc, ni, nto) profile over the coarse channels of every bank
  return fold_run(nbank, in, nchan, nif, ntime, win, nfpc, tavby, op, mask, mask_ld, out, kept,
                  nfpc, nfpc * d[1], stream);
}

// Checks and args of an unfold (every entry point); out: bank b's channel c at
// out[b*nc + c + i*out_ld_i + t*out_ld_t].
static int unfold_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                          int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby, int uop,
                          const float *prof, int64_t prof_ld_i, int64_t prof_ld_t, float *out,
                          int64_t out_ld_i, int64_t out_ld_t, bool query, UnfoldArgs *ap,
                          int64_t *grid, bool *empty) {
  Geo g;
  int64_t J, T;
  int rc = fold_geometry(nbank, nchan, nif, ntime, win, nfpc, tavby, &g, &J, &T);
  if (rc) return rc;
  static const char what[] = "unfold: ";
  if (uop != BLDP_UNFOLD_DIV && uop != BLDP_UNFOLD_SUB)
    return fail(BLDP_EINVAL, "unfold: op %d is not divide (%d) or subtract (%d)", uop,
                BLDP_UNFOLD_DIV, BLDP_UNFOLD_SUB);
  UnfoldArgs &a = *ap;
  a = UnfoldArgs{};
  a.prof = prof, a.out = out;
  a.prof_ld_i = prof_ld_i, a.prof_ld_t = prof_ld_t, a.out_ld_i = out_ld_i, a.out_ld_t = out_ld_t;
  a.nc = g.nc, a.ni = g.ni, a.nt = g.nt, a.nfpc = nfpc, a.T = T;
  a.sub = uop == BLDP_UNFOLD_SUB;
  *empty = g.nc == 0 || g.ni == 0 || g.nt == 0;
  rc = set_window(what, a, g, nbank, in);
  if (rc) return rc;
  const int64_t nto = g.nt / T;
  const bool pitch4 = (g.ni <= 1 || (prof_ld_i % 4 == 0 && out_ld_i % 4 == 0)) &&
                      (nto <= 1 || prof_ld_t % 4 == 0) && (g.nt <= 1 || out_ld_t % 4 == 0);
  *grid = plan_unfold(a, fold_vec_ok(nbank, in, g) && aligned16(prof) && aligned16(out) && pitch4);
  if (query || *empty) return BLDP_OK;
  rc = check_banks(what, nbank, in);
  if (rc) return rc;
  if (!prof) return fail(BLDP_EINVAL, "unfold: null profile pointer");
  if (!out) return fail(BLDP_EINVAL, "unfold: null output pointer");
  if (prof_ld_i < 0 || prof_ld_t < 0)
    return fail(BLDP_EINVAL, "unfold: profile strides (%lld, %lld) are negative",
                (long long)prof_ld_i, (long long)prof_ld_t);
  const int64_t NC = nbank * g.nc;
  rc = check_out_strides(what, 1, 0, out_ld_i, out_ld_t, NC, g.ni, g.nt);
  if (rc) return rc;
  // (the wording of the overlap with the window is the unfold's own)
  int64_t lo;
  size_t wbytes;
  window_span(g, &lo, &wbytes);
  const size_t obytes = 4 * (size_t)((NC - 1) + (g.ni - 1) * out_ld_i + (g.nt - 1) * out_ld_t + 1);
  const size_t pbytes =
      4 * (size_t)((nfpc - 1) + (g.ni - 1) * prof_ld_i + (nto - 1) * prof_ld_t + 1);
  for (int b = 0; b < nbank; ++b)
    if (spans_overlap(out, obytes, in[b] + lo, wbytes))
      return fail(BLDP_EINVAL, "unfold: out overlaps the input window (bank %d); the unfold is "
                  "not in place", b);
  if (spans_overlap(out, obytes, prof, pbytes))
    return fail(BLDP_EINVAL, "unfold: out overlaps the profile");
  return BLDP_OK;
}

static int unfold_run(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                      int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby, int uop,
                      const float *prof, int64_t prof_ld_i, int64_t prof_ld_t, float *out,
                      int64_t out_ld_i, int64_t out_ld_t, void *stream) {
  UnfoldArgs a;
  int64_t grid = 0;
  bool empty = false;
  int rc = unfold_prepare(nbank, in, nchan, nif, ntime, win, nfpc, tavby, uop, prof, prof_ld_i,
                          prof_ld_t, out, out_ld_i, out_ld_t, false, &a, &grid, &empty);
  if (rc || empty) return rc;
  hipStream_t s = (hipStream_t)stream;
  return run_planned("unfold", 0, s, [&](void *) { return launch_unfold(a, grid, s); });
}

int bldp_unfold_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                         const int64_t *win, int64_t nfpc, int64_t tavby, const float *prof,
                         int64_t prof_ld_i, int64_t prof_ld_t, const float *out, int64_t out_ld_i,
                         int64_t out_ld_t, int64_t info[4]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  UnfoldArgs a;
  int64_t grid = 0;
  bool empty = false;
  const float *ins[1] = {in};
  int rc = unfold_prepare(1, ins, nchan, nif, ntime, win, nfpc, tavby, BLDP_UNFOLD_DIV, prof,
                          prof_ld_i, prof_ld_t, const_cast<float *>(out), out_ld_i, out_ld_t, true,
                          &a, &grid, &empty);
  if (rc) return rc;
  info[0] = empty ? 0 : a.vec;
  info[1] = empty ? 0 : grid;
  info[2] = empty ? 0 : (a.vec ? 4 : 1);
  info[3] = 0;
  return BLDP_OK;
}

int bldp_unfold_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, int64_t nfpc, int64_t tavby, int uop, const float *prof,
                    int64_t prof_ld_i, int64_t prof_ld_t, float *out, int64_t out_ld_i,
                    int64_t out_ld_t, void *stream) {
  const float *ins[1] = {in};
  return unfold_run(1, ins, nchan, nif, ntime, win, nfpc, tavby, uop, prof, prof_ld_i, prof_ld_t,
                    out, out_ld_i, out_ld_t, stream);
}

int bldp_band_unfold_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby, int uop,
                         const float *prof, int64_t prof_ld_i, int64_t prof_ld_t, float *out,
                         void *stream) {
  int64_t l[4];  // (the dense vcat of the banks' windows)
  const int rc = band_layout(nbank, nchan, nif, ntime, win, 1, 1, l);
  if (rc) return rc;
  return unfold_run(nbank, in, nchan, nif, ntime, win, nfpc, tavby, uop, prof, prof_ld_i, prof_ld_t,
                    out, l[1], l[2], stream);
}

// ---- dedoppler: the drift-rate sums of every channel ---------------------------
// Checks, window and plan of a dedoppler (every entry point).  l = {out_bank,
// out_ld_i, out_ld_t, out_ld_q}: output (c, i, b) of bank k at [k*l[0] + c + i*l[1]
// + b*l[2]], drift plane q of sums at + q*l[3].  query: the plan call.
static int dedop_prepare(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int64_t tavby, int64_t maxdrift,
                         int64_t seg, float *best, int *drift, float *sums, const int64_t l[4],
                         bool query, DedopArgs *ap, Plan *pp, bool *empty) {
  static const char what[] = "dedoppler: ";
  int rc = check_nbank(nbank);
  if (rc) return rc;
  if (tavby < 2)
    return fail(BLDP_EINVAL, "dedoppler: tavby=%lld: a block needs two spectra", (long long)tavby);
  if (tavby > ((int64_t)1 << 20))
    return fail(BLDP_EINVAL, "dedoppler: tavby=%lld beyond 2^20", (long long)tavby);
  if (maxdrift < 0 || maxdrift > BLDP_MAX_DRIFT)
    return fail(BLDP_EINVAL, "dedoppler: maxdrift=%lld outside 0..%d", (long long)maxdrift,
                BLDP_MAX_DRIFT);
  if (seg < 0) return fail(BLDP_EINVAL, "dedoppler: seg=%lld is negative", (long long)seg);
  Geo g;
  int64_t F, T;
  rc = resolve_blocks(nchan, nif, ntime, win, 1, tavby, &g, &F, &T);
  if (rc) return rc;
  DedopArgs &a = *ap;
  a = DedopArgs{};
  a.best = best, a.drift = drift, a.sums = sums;
  a.out_bank = l[0], a.out_ld_i = l[1], a.out_ld_t = l[2], a.out_ld_q = l[3];
  a.nc = g.nc, a.ni = g.ni, a.nb = g.nt / T, a.T = T;
  a.seg = seg, a.D = (int32_t)maxdrift;
  *empty = g.nc == 0 || g.ni == 0 || g.nt == 0;
  bool words, rows16;
  rc = set_window(what, a, g, nbank, in, &words, &rows16);
  if (!rc) rc = plan_dedoppler(a, rows16 && vec_ok(g), pp);
  if (rc || query || *empty) return rc;
  rc = check_banks(what, nbank, in);
  if (rc) return rc;
  if ((best == nullptr) != (drift == nullptr))
    return fail(BLDP_EINVAL, "dedoppler: best and drift go together");
  if (!best && !sums) return fail(BLDP_EINVAL, "dedoppler: best / drift and sums are all null");
  rc = check_out_strides(what, nbank, l[0], l[1], l[2], a.nc, a.ni, a.nb);
  if (rc) return rc;
  const int64_t K = 2 * maxdrift + 1;
  const int64_t plane = (nbank - 1) * l[0] + (a.nc - 1) + (a.ni - 1) * l[1] + (a.nb - 1) * l[2] + 1;
  if (sums && K > 1 && l[3] < plane)
    return fail(BLDP_EINVAL, "dedoppler: sums planes %lld elements apart overlap for a (%lld, %lld, "
                "%lld) plane with strides (%lld, %lld)", (long long)l[3], (long long)(nbank * a.nc),
                (long long)a.ni, (long long)a.nb, (long long)l[1], (long long)l[2]);
  const Span outs[3] = {{best, 4 * (size_t)plane, "best"},
                        {drift, 4 * (size_t)plane, "drift"},
                        {sums, 4 * (size_t)((K - 1) * l[3] + plane), "sums"}};
  return check_disjoint(what, outs, 3, g, nbank, in, {nullptr, 0, ""});
}

static int dedop_run(int nbank, const float *const *in, int64_t nchan, int64_t nif, int64_t ntime,
                     const int64_t *win, int64_t tavby, int64_t maxdrift, int64_t seg, float *best,
                     int *drift, float *sums, const int64_t l[4], void *stream) {
  DedopArgs a;
  Plan p;
  bool empty = false;
  int rc = dedop_prepare(nbank, in, nchan, nif, ntime, win, tavby, maxdrift, seg, best, drift,
                         sums, l, false, &a, &p, &empty);
  if (rc || empty) return rc;
  hipStream_t s = (hipStream_t)stream;
  return run_planned("dedoppler", 0, s, [&](void *) { return launch_dedoppler(a, p, s); });
}

int bldp_dedoppler_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                            const int64_t *win, int64_t tavby, int64_t maxdrift, int64_t seg,
                            int64_t info[10]) {
  if (!info) return fail(BLDP_EINVAL, "null info");
  DedopArgs a;
  Plan p;
  bool empty = false;
  const float *ins[1] = {in};
  const int64_t l[4] = {0, 0, 0, 0};
  int rc = dedop_prepare(1, ins, nchan, nif, ntime, win, tavby, maxdrift, seg, nullptr, nullptr,
                         nullptr, l, true, &a, &p, &empty);
  if (rc) return rc;
  for (int q = 0; q < 10; ++q) info[q] = 0;
  if (empty) return BLDP_OK;  // (nothing is launched)
  info[0] = p.path;
  info[1] = a.C;
  info[2] = a.H;
  info[3] = a.R;
  info[4] = dedoppler_group();
  info[5] = p.nrw;
  info[6] = p.shm;
  info[7] = p.grid;
  info[8] = a.vec;
  info[9] = (int64_t)p.ws_bytes;
  return BLDP_OK;
}

int bldp_dedoppler_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                       const int64_t *win, int64_t tavby, int64_t maxdrift, int64_t seg,
                       float *best, int *drift, float *sums, int64_t out_ld_i,
                       int64_t out_ld_t, int64_t out_ld_q, void *stream) {
  const float *ins[1] = {in};
  const int64_t l[4] = {0, out_ld_i, out_ld_t, out_ld_q};
  return dedop_run(1, ins, nchan, nif, ntime, win, tavby, maxdrift, seg, best, drift, sums, l,
                   stream);
}

int bldp_band_dedoppler_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                            int64_t ntime, const int64_t *win, int64_t tavby, int64_t maxdrift,
                            int64_t seg, float *best, int *drift, float *sums, void *stream) {
  if (tavby < 2)  // (band_layout reads a tavby below 2 as no blocks at all)
    return fail(BLDP_EINVAL, "dedoppler: tavby=%lld: a block needs two spectra", (long long)tavby);
  int64_t l[4];
  const int rc = band_layout(nbank, nchan, nif, ntime, win, 1, tavby, l);
  if (rc) return rc;
  return dedop_run(nbank, in, nchan, nif, ntime, win, tavby, maxdrift, seg, best, drift, sums, l,
                   stream);
}

int bldp_reduce_out_dtype(int dtype, int op) {
  const int d = typed_out_dtype(dtype, op);
  if (d < 0) return fail(BLDP_EINVAL, "unknown element type %d or op %d", dtype, op);
  return d;
}

}  // extern "C"

namespace {
// The TypedArgs of a typed reduce (bldp_reduce_strided's checks); *empty when
// there is nothing to do.
int typed_reduce_args(int dtype, const void *in, int64_t nchan, int64_t nif, int64_t ntime,
                      const int64_t *win, int64_t fqavby, int64_t tavby, int op, void *out,
                      int64_t out_ld_i, int64_t out_ld_t, TypedArgs *ap, bool *empty) {
  if (!dtype_size(dtype)) return fail(BLDP_EINVAL, "unknown element type %d", dtype);
  if (!valid_op(op)) return fail(BLDP_EINVAL, "unknown op %d (" BLDP_OP_NAMES ")", op);
  if (stat_op(op))
    return fail(BLDP_EINVAL, "median/var/std/mad take Float32 on the GPU (element type %d)", dtype);
  Geo g;
  int rc = resolve_window(nchan, nif, ntime, win, &g);
  if (rc) return rc;
  int64_t F, T;
  rc = resolve_factors(g, fqavby, tavby, &F, &T);
  if (rc) return rc;
  TypedArgs &a = *ap;
  a = TypedArgs{};
  a.dtype = dtype;
  a.nbank = 1;
  a.in[0] = in;
  a.out = out;
  a.out_ld_i = out_ld_i;
  a.out_ld_t = out_ld_t;
  a.in_off = g.off;
  a.in_cs = g.cs;
  a.in_ld_i = g.ld_i;
  a.in_ld_t = g.ld_t;
  a.nco = g.nc / F;
  a.ni = g.ni;
  a.nto = g.nt / T;
  a.F = F;
  a.T = T;
  a.num_cus = num_cus_current();
  *empty = a.nco * a.ni * a.nto == 0;
  if (*empty) return BLDP_OK;
  if (!in || !out) return fail(BLDP_EINVAL, "null pointer");
  return BLDP_OK;
}

// The TypedArgs of a typed getkurtosis (bldp_kurtosis's checks).
int typed_kurt_args(int dtype, const void *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, double *out, TypedArgs *ap, bool *empty) {
  if (!dtype_size(dtype)) return fail(BLDP_EINVAL, "unknown element type %d", dtype);
  Geo g;
  int rc = resolve_window(nchan, nif, ntime, win, &g);
  if (rc) return rc;
  TypedArgs &a = *ap;
  a = TypedArgs{};
  a.dtype = dtype;
  a.nbank = 1;
  a.in[0] = in;
  a.out = out;
  a.in_off = g.off;
  a.in_cs = g.cs;
  a.in_ld_i = g.ld_i;
  a.in_ld_t = g.ld_t;
  a.nco = g.nc;
  a.ni = g.ni;
  a.nto = g.nt;
  a.F = a.T = 1;
  a.num_cus = num_cus_current();
  *empty = a.nco * a.ni == 0;
  if (*empty) return BLDP_OK;
  if (!out || (!in && g.nt > 0)) return fail(BLDP_EINVAL, "null pointer");
  return BLDP_OK;
}
}  // namespace

extern "C" {

int bldp_reduce_strided(int dtype, const void *in, int64_t nchan, int64_t nif, int64_t ntime,
                        const int64_t *win, int64_t fqavby, int64_t tavby, int op, void *out,
                        int64_t out_ld_i, int64_t out_ld_t, void *stream) {
  if (dtype == BLDP_DT_F32)
    return bldp_reduce_strided_f32(static_cast<const float *>(in), nchan, nif, ntime, win, fqavby,
                                   tavby, op, static_cast<float *>(out), out_ld_i, out_ld_t,
                                   stream);
  TypedArgs a;
  bool empty = false;
  int rc = typed_reduce_args(dtype, in, nchan, nif, ntime, win, fqavby, tavby, op, out, out_ld_i,
                             out_ld_t, &a, &empty);
  if (rc || empty) return rc;
  hipError_t e = launch_reduce_typed(a, op, (hipStream_t)stream);
  if (e != hipSuccess) return fail(BLDP_EHIP, "typed reduce launch: %s", hipGetErrorString(e));
  return BLDP_OK;
}

int bldp_kurtosis(int dtype, const void *in, int64_t nchan, int64_t nif, int64_t ntime,
                  const int64_t *win, double *out, void *stream) {
  if (dtype == BLDP_DT_F32)
    return bldp_kurtosis_f32(static_cast<const float *>(in), nchan, nif, ntime, win, out, nullptr,
                             stream);
  TypedArgs a;
  bool empty = false;
  int rc = typed_kurt_args(dtype, in, nchan, nif, ntime, win, out, &a, &empty);
  if (rc || empty) return rc;
  ScratchLease lease;  // time-chunk partial sums (k_kurt_i8), held until queued
  if (const size_t wsb = kurtosis_typed_ws_bytes(a)) {
    rc = scratch_lease((hipStream_t)stream, wsb, &lease);
    if (rc) return rc;
    a.ws = lease.ptr;
    a.ws_bytes = wsb;
  }
  hipError_t e = launch_kurtosis_typed(a, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(BLDP_EHIP, "typed kurtosis launch: %s", hipGetErrorString(e));
  return BLDP_OK;
}

// bldp_reduce_strided / bldp_kurtosis prepared once (any element type): a
// launch through bldp_reduce_launch is one kernel launch (two for the typed
// getkurtosis of long rows), no argument handling.
int bldp_reduce_prepare(int dtype, const void *in, int64_t nchan, int64_t nif, int64_t ntime,
                        const int64_t *win, int64_t fqavby, int64_t tavby, int op, void *out,
                        int64_t out_ld_i, int64_t out_ld_t, bldp_reduce_op_t *handle) {
  if (!handle) return fail(BLDP_EINVAL, "null handle pointer");
  *handle = nullptr;
  auto *h = new (std::nothrow) bldp_reduce_op{};
  if (!h) return fail(BLDP_ENOMEM, "out of host memory");
  int rc;
  if (dtype == BLDP_DT_F32) {
    h->kind = bldp_reduce_op::F32_REDUCE;
    const float *ins[1] = {static_cast<const float *>(in)};
    rc = prepare_reduce(1, ins, nchan, nif, ntime, win, fqavby, tavby, op,
                        static_cast<float *>(out), 0, out_ld_i, out_ld_t, false, false, &h->a,
                        &h->p, &h->empty);
  } else {
    h->kind = bldp_reduce_op::TYPED_REDUCE;
    rc = typed_reduce_args(dtype, in, nchan, nif, ntime, win, fqavby, tavby, op, out, out_ld_i,
                           out_ld_t, &h->t, &h->empty);
  }
  if (rc == BLDP_OK && hipGetDevice(&h->dev) != hipSuccess)
    rc = fail(BLDP_EHIP, "hipGetDevice failed");
  if (rc) {
    delete h;
    return rc;
  }
  h->op = op;
  *handle = h;
  return BLDP_OK;
}

int bldp_kurtosis_prepare(int dtype, const void *in, int64_t nchan, int64_t nif, int64_t ntime,
                          const int64_t *win, double *out, bldp_reduce_op_t *handle) {
  if (!handle) return fail(BLDP_EINVAL, "null handle pointer");
  *handle = nullptr;
  auto *h = new (std::nothrow) bldp_reduce_op{};
  if (!h) return fail(BLDP_ENOMEM, "out of host memory");
  int rc;
  if (dtype == BLDP_DT_F32) {
    h->kind = bldp_reduce_op::F32_KURT;
    const float *ins[1] = {static_cast<const float *>(in)};
    rc = kurt_setup(1, ins, nchan, nif, ntime, win, &h->k, 4);
    h->empty = false;
  } else {
    h->kind = bldp_reduce_op::TYPED_KURT;
    rc = typed_kurt_args(dtype, in, nchan, nif, ntime, win, out, &h->t, &h->empty);
  }
  if (rc == BLDP_OK && hipGetDevice(&h->dev) != hipSuccess)
    rc = fail(BLDP_EHIP, "hipGetDevice failed");
  if (rc) {
    delete h;
    return rc;
  }
  h->kout = out;
  h->op = 0;
  *handle = h;
  return BLDP_OK;
}

int bldp_fqav_range(double first, double step, int64_t len, int64_t n, double *out_first,
                    double *out_step, int64_t *out_len) {
  if (!out_first || !out_step || !out_len) return fail(BLDP_EINVAL, "null pointer");
  if (len < 0) return fail(BLDP_EINVAL, "negative range length");
  if (n <= 1) {  // src/gbtworkerfunctions.jl:28
    *out_first = first;
    *out_step = step;
    *out_len = len;
    return BLDP_OK;
  }
  *out_first = first + (double)(n - 1) * step / 2.0;  // :29
  *out_step = (double)n * step;                        // :30
  *out_len = len / n;                                  // :31 (floor)
  return BLDP_OK;
}

int bldp_unchunk_f32(const float *packed, const int64_t chunk[3], const int64_t box0[3],
                     const int64_t grid[3], const int64_t *win, float *out, void *stream) {
  if (!chunk || !box0 || !grid || !win) return fail(BLDP_EINVAL, "null pointer");
  UnchunkArgs u{chunk[0], chunk[1], chunk[2], box0[0], box0[1], box0[2], grid[0], grid[1],
                grid[2], win[0], win[1], win[2], win[3], win[4], win[5], win[6], win[7], win[8]};
  if (u.ct <= 0 || u.ci <= 0 || u.cc <= 0 || u.gt <= 0 || u.gi <= 0 || u.gc <= 0)
    return fail(BLDP_EINVAL, "bad chunk geometry");
  // every window element must fall inside the chunk box (no out-of-range reads)
  const int64_t ext[3][3] = {{u.c0, u.nc, u.cs}, {u.i0, u.ni, u.is}, {u.t0, u.nt, u.ts}};
  const int64_t lo[3] = {u.bc0, u.bi0, u.bt0}, len[3] = {u.gc * u.cc, u.gi * u.ci, u.gt * u.ct};
  for (int a = 0; a < 3; ++a) {
    if (ext[a][1] < 0) return fail(BLDP_EINVAL, "negative window count");
    if (ext[a][1] == 0) return BLDP_OK;
    // counts and steps beyond the box cannot stay inside it; checked first so
    // the last-index product below cannot overflow
    if (ext[a][1] > 1 && (ext[a][1] > len[a] || ext[a][2] > len[a] || ext[a][2] < -len[a]))
      return fail(BLDP_EBOUNDS, "window axis %d outside the decoded chunk box", a + 1);
    const int64_t first = ext[a][0], last = ext[a][0] + (ext[a][1] - 1) * ext[a][2];
    if (std::min(first, last) < lo[a] || std::max(first, last) >= lo[a] + len[a])
      return fail(BLDP_EBOUNDS, "window axis %d outside the decoded chunk box", a + 1);
  }
  if (!packed || !out) return fail(BLDP_EINVAL, "null pointer");
  hipError_t e = launch_unchunk(packed, u, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(BLDP_EHIP, "unchunk launch: %s", hipGetErrorString(e));
  return BLDP_OK;
}

int bldp_synth_f32(float *out, int64_t nchan, int64_t nif, int64_t ntime, int64_t nfpc,
                   uint64_t seed, int kind, void *stream) {
  if (nchan < 0 || nif < 0 || ntime < 0) return fail(BLDP_EINVAL, "negative dimension");
  if (kind != 0 && kind != 1) return fail(BLDP_EINVAL, "unknown synth kind %d", kind);
  if (nfpc < 1) return fail(BLDP_EINVAL, "nfpc must be >= 1");
  if (nchan * nif * ntime > 0 && !out) return fail(BLDP_EINVAL, "null pointer");
  hipError_t e = launch_synth(out, nchan, nif, ntime, nfpc, seed, kind, (hipStream_t)stream);
  if (e != hipSuccess) return fail(BLDP_EHIP, "synth launch: %s", hipGetErrorString(e));
  return BLDP_OK;
}

}  // extern "C"
