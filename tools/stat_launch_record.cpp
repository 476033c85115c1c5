// stat_launch_record — what the planners and dispatchers of stats.hip and
// tstats.hip do (var, std, median, mad, quantile, quantiles and outliers over
// blocks of channels and over blocks of spectra), recorded on the host: the host
// halves of the two files linked into this program, which stands in for the few
// HIP runtime entry points they call.  The device code the objects would
// register is absent: its __hip_fatbin_* symbols are defined as 0 at link time.
// It needs no GPU and no HIP runtime library and is never loaded into Python.
// tests/test_stat_reach_host.py's `tool` fixture is the build recipe (three
// --cuda-host-only compiles and one link) and runs it.
//
// What api.hip decides before the two files see a call is restated here:
// resolve_window, resolve_factors, set_blocks and the dense / stitched result
// layouts, `words` (every bank pointer dword-aligned: a field of the case),
// quantile_rank and quantile_set (host.hip), the plan words of fill_reduce_info
// and fill_tstat_info with what the quantile, quantiles and outliers plan
// queries put beside them, on 256 CUs in 8 XCDs.  tests/test_stat_reach_host.py
// holds that restatement to the library's own plan entry points.  The split of
// more than BLDP_MAX_QUANTILES probabilities into several launches is the
// engine's: a case holds at most that many.
//
// Usage: stat_launch_record --list    every registered entry point of the two
//          files, one per line
//        stat_launch_record --reach   a sweep over block lengths on both sides
//          of every switch of plan_stats, plan_tstat, plan_tstat_q and the
//          launchers; channel steps 1, 2 and -1, a start off a 16-byte boundary,
//          bank pointers that are and are not dword-aligned; blocks, channels,
//          IFs and banks; every op, quantiles with 1 to 8 distinct lower ranks,
//          outliers with and without a mask.  Prints, per entry point started,
//          the smallest input (elements per bank) that started it, as a line
//          --cases takes
//        stat_launch_record --cases   what each case read from stdin runs, one
//          case per line:
//            NCHAN NIF NTIME WINDOW AXIS N NBANK WORDS OP
//          WINDOW is - or nine comma-separated integers (start, count, step of
//          the channel, IF and time axes, 0-based).  AXIS 0: blocks of N
//          channels (bldp_reduce_* with fqavby = N, bldp_quantile*_ and
//          bldp_outliers_* with axis 0); AXIS 2: blocks of N spectra
//          (bldp_tstat_* and the same with axis 2).  OP is var, std, median,
//          mad, quantile:P, quantiles:P1,P2,... or outliers:MASK (1: a mask is
//          written).  Printed per case: plan=, the ten plan words of ONE bank as
//          the op's plan entry point reports them (eight for the four plain
//          ops, then zeros), and every symbol launched, in order, with grid and
//          block.
#include <cxxabi.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "bldp_impl.h"

namespace {

struct Launch {
  const void *fn;
  dim3 grid, block;
};
std::vector<Launch> g_launches;

std::map<const void *, std::string> &names() {
  static std::map<const void *, std::string> m;  // (filled by static constructors)
  return m;
}

// "void bldp::(anonymous namespace)::k_mom_lanes<16, true>(bldp::RedArgs, int)" ->
// "k_mom_lanes<16,true>"; enumerators lose their cast: "(bldp::Sel)2" -> "2"
std::string short_name(const char *mangled) {
  int st = 0;
  char *d = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
  std::string s = st == 0 && d ? d : mangled;
  free(d);
  const size_t k = s.find("k_");
  if (k != std::string::npos) s = s.substr(k);
  for (size_t c; (c = s.find("(bldp::Sel)")) != std::string::npos;) s.erase(c, 11);
  const size_t par = s.find('(');  // (the parameter list)
  if (par != std::string::npos) s = s.substr(0, par);
  // the trailing pack of the SEL_QUANTILES / SEL_OUTLIERS forms: ", bldp::QSet>" -> ">"
  for (const char *t : {",bldp::QSet", ",bldp::OutlArgs"}) {
    std::string o;
    for (char c : s)
      if (c != ' ') o += c;
    s = o;
    const size_t at = s.find(t);
    if (at != std::string::npos) s.erase(at, strlen(t));
  }
  return s;
}

hipError_t record(const void *fn, dim3 grid, dim3 block) {
  g_launches.push_back(Launch{fn, grid, block});
  return hipSuccess;
}

struct CallConfig {
  dim3 grid, block;
  size_t shm;
  hipStream_t stream;
};
thread_local CallConfig t_cfg;

}  // namespace

// The runtime entry points the host halves of stats.hip and tstats.hip call.
extern "C" {
void **__hipRegisterFatBinary(const void *) {
  static void *handle = nullptr;
  return &handle;
}
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name,
                           unsigned, void *, void *, void *, void *, int *) {
  names()[host_fn] = short_name(device_name);
}
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shm, hipStream_t stream) {
  t_cfg = CallConfig{grid, block, shm, stream};
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shm, hipStream_t *stream) {
  *grid = t_cfg.grid;
  *block = t_cfg.block;
  *shm = t_cfg.shm;
  *stream = t_cfg.stream;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **, size_t, hipStream_t) {
  return record(fn, grid, block);
}
hipError_t hipExtLaunchKernel(const void *fn, dim3 grid, dim3 block, void **, size_t, hipStream_t,
                              hipEvent_t, hipEvent_t, int) {
  return record(fn, grid, block);
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
}

namespace bldp {
int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  return code;
}
// (kernels.hip's: no launch here carries timing events)
void take_launch_events(hipEvent_t *start, hipEvent_t *stop) { *start = *stop = nullptr; }
}  // namespace bldp

// host.hip's quantile_rank and quantile_set, restated (the declarations are bldp_impl.h's).
void bldp::quantile_rank(int64_t n, double p, int64_t *rank, double *g) {
#pragma clang fp contract(off)
  const double m = 1.0 + p * (1.0 - 1.0 - 1.0);
  const double np = (double)n * p;
  const double aleph = np + m;
  const double j = std::min(std::max(std::trunc(aleph), 1.0), (double)(n - 1));
  *rank = (int64_t)j - 1;
  *g = std::min(std::max(aleph - j, 0.0), 1.0);
}
void bldp::quantile_set(int64_t n, int np, const double *p, int64_t out_ld_q, QSet *qs) {
  QSet s{};
  s.np = np;
  s.out_ld_q = out_ld_q;
  int32_t lower[BLDP_MAX_QUANTILES], all[2 * BLDP_MAX_QUANTILES];
  for (int k = 0; k < np; ++k) {
    int64_t r;
    quantile_rank(n, p[k], &r, &s.g[k]);
    lower[k] = (int32_t)r;
    s.low[k] = lower[k];
    all[2 * k] = lower[k];
    all[2 * k + 1] = lower[k] + 1;
  }
  std::sort(all, all + 2 * np);
  s.nr = (int32_t)(std::unique(all, all + 2 * np) - all);
  std::copy(all, all + s.nr, s.rank);
  std::sort(s.low, s.low + np);
  s.nlow = (int32_t)(std::unique(s.low, s.low + np) - s.low);
  std::fill(s.low + s.nlow, s.low + BLDP_MAX_QUANTILES, 0);
  for (int k = 0; k < np; ++k) {
    s.lo[k] = (uint8_t)(std::lower_bound(s.rank, s.rank + s.nr, lower[k]) - s.rank);
    s.hi[k] = (uint8_t)(std::lower_bound(s.rank, s.rank + s.nr, lower[k] + 1) - s.rank);
    s.lsel[k] = (uint8_t)(std::lower_bound(s.low, s.low + s.nlow, lower[k]) - s.low);
  }
  *qs = s;
}

namespace {

using bldp::OutlArgs;
using bldp::Plan;
using bldp::QSet;
using bldp::RedArgs;
using bldp::TStatArgs;
using bldp::TStatPlan;
using bldp::quantile_rank;
using bldp::quantile_set;

constexpr int kNumCus = 256;
constexpr int kXcdLg = 3;

bool is_stat_symbol(const std::string &s) {
  for (const char *p : {"k_mom_", "k_median_", "k_quantiles_", "k_tstat_", "k_tquantiles_"})
    if (s.rfind(p, 0) == 0) return true;
  return false;
}
const char *sym_of(const void *fn) {
  const auto it = names().find(fn);
  return it == names().end() ? "?" : it->second.c_str();
}

// banks that are (words) or are not dword-aligned; never dereferenced
const float *fake_in(int b, bool words) {
  return (const float *)(uintptr_t)(0x100000000ull + 0x10000000ull * b + (words ? 0 : 2));
}
template <class T>
T *fake_out(int q) {
  return (T *)(uintptr_t)(0x7000000000ull + 0x100000000ull * q);
}

// api.hip's resolve_window, restated.
struct Geo {
  int64_t nc, ni, nt;
  int64_t off, cs, ld_i, ld_t;
};
bool resolve_window(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, Geo *g) {
  if (nchan < 0 || nif < 0 || ntime < 0) return false;
  const int64_t dims[3] = {nchan, nif, ntime};
  int64_t start[3], count[3], step[3];
  for (int ax = 0; ax < 3; ++ax) {
    start[ax] = win ? win[3 * ax] : 0;
    count[ax] = win ? win[3 * ax + 1] : dims[ax];
    step[ax] = win ? win[3 * ax + 2] : 1;
    if (count[ax] < 0) return false;
    if (count[ax] > 0) {
      if (step[ax] == 0) return false;
      const int64_t last = start[ax] + (count[ax] - 1) * step[ax];
      if (start[ax] < 0 || start[ax] >= dims[ax] || last < 0 || last >= dims[ax]) return false;
    }
  }
  g->nc = count[0], g->ni = count[1], g->nt = count[2];
  const bool empty = g->nc == 0 || g->ni == 0 || g->nt == 0;
  g->off = empty ? 0 : start[0] + nchan * (start[1] + nif * start[2]);
  g->cs = step[0];
  g->ld_i = nchan * step[1];
  g->ld_t = nchan * nif * step[2];
  return true;
}

enum OpKind { K_VAR, K_STD, K_MEDIAN, K_MAD, K_QUANTILE, K_QUANTILES, K_OUTLIERS };

struct Case {
  int64_t nchan, nif, ntime;
  bool has_win;
  int64_t win[9];
  int axis;
  int64_t n;
  int nbank;
  bool words;
  OpKind kind;
  int np;                         // quantile: 1; quantiles: 1 .. BLDP_MAX_QUANTILES
  double p[BLDP_MAX_QUANTILES];
  bool mask;                      // outliers
};

int op_code(OpKind k) {
  switch (k) {
    case K_VAR: return BLDP_OP_VAR;
    case K_STD: return BLDP_OP_STD;
    case K_MEDIAN: return BLDP_OP_MEDIAN;
    case K_MAD: return BLDP_OP_MAD;
    case K_QUANTILE: return bldp::kOpQuantile;
    case K_QUANTILES: return bldp::kOpQuantiles;
    case K_OUTLIERS: return BLDP_OP_MAD;
  }
  return -1;
}

template <class A>
void set_window(A &a, const Geo &g, int nbank, bool words) {
  a.nbank = nbank;
  a.in_off = g.off, a.in_cs = g.cs, a.in_ld_i = g.ld_i, a.in_ld_t = g.ld_t;
  for (int b = 0; b < nbank; ++b) a.in[b] = fake_in(b, words);
}

// Blocks of channels: prepare_reduce's stat branch for nbank banks (dense for
// one, the vcat of the banks for more), the plan words, and with `run` the launch.
bool call_axis0(const Case &c, const Geo &g, int nbank, bool run, int64_t info[10]) {
  const int64_t F = c.n <= 1 ? 1 : c.n;
  if (g.nc % F != 0) return false;
  if (c.kind == K_OUTLIERS && c.n < 2) return false;
  if (c.kind == K_QUANTILES && c.n <= 1) return false;  // (np copies of the window: the median's F = 1)
  RedArgs a{};
  if (c.kind == K_QUANTILE && F > 1) {
    int64_t q;
    quantile_rank(F, c.p[0], &q, &a.qg);
    a.qrank = (int32_t)q;
  }
  const int64_t d[3] = {g.nc / F, g.ni, g.nt};
  a.nco = d[0], a.ni = d[1], a.nto = d[2], a.F = F, a.T = 1;
  a.out_bank = nbank > 1 ? d[0] : d[0] * d[1] * d[2];
  a.out_ld_i = nbank * d[0];
  a.out_ld_t = nbank * d[0] * d[1];
  if (a.nco == 0 || a.ni == 0 || a.nto == 0) return false;
  a.out = c.kind == K_OUTLIERS ? nullptr : fake_out<float>(0);
  set_window(a, g, nbank, c.words);
  Plan p;
  if (bldp::plan_stats(a, op_code(c.kind), c.words && g.cs == 1, kXcdLg, &p) != BLDP_OK)
    return false;
  if (info) {
    info[0] = p.path, info[1] = p.lpg, info[2] = a.ts, info[3] = a.k4, info[4] = a.nchunk;
    info[5] = p.grid, info[6] = (int64_t)p.ws_bytes, info[7] = a.vec_out;
    info[8] = info[9] = 0;
    if (c.kind == K_QUANTILE) info[6] = F > 1 ? a.qrank : -1;
  }
  QSet qs{};
  if (c.kind == K_QUANTILES) {
    quantile_set(c.n, c.np, c.p, a.out_ld_t * d[2], &qs);
    if (info) info[8] = qs.nr, info[9] = bldp::stats_q_reads(p);
  }
  if (c.kind == K_OUTLIERS && info)
    info[8] = bldp::stats_outl_reads(p, c.mask), info[9] = c.mask ? 1 : 0;
  if (!run) return true;
  if (c.kind == K_QUANTILES) return bldp::launch_stats_q(a, p, qs, nullptr) == hipSuccess;
  if (c.kind == K_OUTLIERS) {
    OutlArgs oa{};
    oa.nsigma = 5.0;
    oa.med = fake_out<float>(1), oa.mad = fake_out<float>(2), oa.count = fake_out<uint32_t>(3);
    oa.mask = c.mask ? fake_out<uint8_t>(4) : nullptr;
    oa.mask_bank = nbank > 1 ? g.nc : 0;
    oa.mask_ld_i = nbank * g.nc;
    oa.mask_ld_t = oa.mask_ld_i * g.ni;
    return bldp::launch_stats_outl(a, p, oa, nullptr) == hipSuccess;
  }
  return bldp::launch_stats(a, p, op_code(c.kind), nullptr) == hipSuccess;
}

// Blocks of spectra: tstat_prepare, and quantiles_run / outliers_run after it.
bool call_axis2(const Case &c, const Geo &g, int nbank, bool run, int64_t info[10]) {
  const int64_t T = c.n;
  if (T <= 1) return false;  // (the window itself: the reduce's copy, not these files)
  if (g.nt % T != 0) return false;
  TStatArgs a{};
  a.nc = g.nc, a.ni = g.ni, a.T = T, a.nb = g.nt / T;
  a.out = c.kind == K_OUTLIERS ? nullptr : fake_out<float>(0);
  a.out_bank = nbank > 1 ? g.nc : 0;
  a.out_ld_i = nbank * g.nc;
  a.out_ld_b = nbank * g.nc * g.ni;
  if (c.kind == K_QUANTILE || c.kind == K_QUANTILES) {  // (quantiles: tstat_prepare with p[0])
    int64_t q;
    quantile_rank(T, c.p[0], &q, &a.qg);
    a.qrank = (int32_t)q;
  }
  if (a.nc == 0 || a.ni == 0 || a.nb == 0) return false;
  set_window(a, g, nbank, c.words);
  TStatPlan p{};
  const int op = c.kind == K_QUANTILES ? bldp::kOpQuantile : op_code(c.kind);
  if (bldp::plan_tstat(a, op, c.words, kNumCus, kXcdLg, &p) != BLDP_OK) return false;
  QSet qs{};
  if (c.kind == K_QUANTILES) {
    quantile_set(T, c.np, c.p, a.out_ld_b * a.nb, &qs);
    if (bldp::plan_tstat_q(a, qs.nlow, c.words, kNumCus, kXcdLg, &p) != BLDP_OK) return false;
  }
  if (info) {
    info[0] = p.path, info[1] = p.cpl, info[2] = p.tsplit, info[3] = p.passes;
    info[4] = p.grid, info[5] = (int64_t)p.ws_bytes, info[6] = a.nb;
    info[7] = p.tsplit > 1 ? ((int64_t)1 << a.lx_log2) : 0;
    info[8] = info[9] = 0;
    if (c.kind == K_QUANTILE) info[5] = a.qrank;
    if (c.kind == K_QUANTILES) info[8] = qs.nr, info[9] = p.passes;
    if (c.kind == K_OUTLIERS) info[8] = bldp::tstat_outl_reads(p, c.mask), info[9] = c.mask ? 1 : 0;
  }
  if (!run) return true;
  if (c.kind == K_QUANTILES) return bldp::launch_tstat_q(a, p, qs, nullptr) == hipSuccess;
  if (c.kind == K_OUTLIERS) {
    OutlArgs oa{};
    oa.nsigma = 5.0;
    oa.med = fake_out<float>(1), oa.mad = fake_out<float>(2), oa.count = fake_out<uint32_t>(3);
    oa.mask = c.mask ? fake_out<uint8_t>(4) : nullptr;
    oa.mask_bank = nbank > 1 ? g.nc : 0;
    oa.mask_ld_i = nbank * g.nc;
    oa.mask_ld_t = oa.mask_ld_i * g.ni;
    return bldp::launch_tstat_outl(a, p, oa, nullptr) == hipSuccess;
  }
  if (p.ws_bytes) a.ws = fake_out<double>(5);
  return bldp::launch_tstat(a, p, op, nullptr) == hipSuccess;
}

// The call of the case: its plan words (of one bank) and, in g_launches, what it
// starts.  False: the API would refuse it, or nothing runs.
bool run_call(const Case &c, int64_t plan[10]) {
  g_launches.clear();
  if (c.nbank < 1 || c.nbank > BLDP_MAX_BANKS || (c.axis != 0 && c.axis != 2)) return false;
  if (c.kind == K_QUANTILE || c.kind == K_QUANTILES) {
    if (c.np < 1 || c.np > BLDP_MAX_QUANTILES) return false;
    for (int k = 0; k < c.np; ++k)
      if (!(c.p[k] >= 0.0 && c.p[k] <= 1.0)) return false;
  }
  Geo g;
  if (!resolve_window(c.nchan, c.nif, c.ntime, c.has_win ? c.win : nullptr, &g)) return false;
  const auto call = c.axis == 0 ? call_axis0 : call_axis2;
  if (!call(c, g, 1, false, plan)) return false;
  return call(c, g, c.nbank, true, nullptr) && !g_launches.empty();
}

const char *kKindNames[] = {"var", "std", "median", "mad", "quantile", "quantiles", "outliers"};

std::string case_line(const Case &c) {
  char buf[1024];
  int n = snprintf(buf, sizeof buf, "%lld %lld %lld ", (long long)c.nchan, (long long)c.nif,
                   (long long)c.ntime);
  if (c.has_win) {
    for (int q = 0; q < 9; ++q)
      n += snprintf(buf + n, sizeof buf - n, "%s%lld", q ? "," : "", (long long)c.win[q]);
  } else {
    n += snprintf(buf + n, sizeof buf - n, "-");
  }
  n += snprintf(buf + n, sizeof buf - n, " %d %lld %d %d %s", c.axis, (long long)c.n, c.nbank,
                (int)c.words, kKindNames[c.kind]);
  if (c.kind == K_QUANTILE || c.kind == K_QUANTILES)
    for (int k = 0; k < c.np; ++k)
      n += snprintf(buf + n, sizeof buf - n, "%s%.17g", k ? "," : ":", c.p[k]);
  if (c.kind == K_OUTLIERS) snprintf(buf + n, sizeof buf - n, ":%d", (int)c.mask);
  return buf;
}

bool parse_op(const std::string &t, Case *c) {
  const size_t col = t.find(':');
  const std::string name = t.substr(0, col);
  int k = -1;
  for (int q = 0; q < 7; ++q)
    if (name == kKindNames[q]) k = q;
  if (k < 0) return false;
  c->kind = (OpKind)k;
  c->np = 0;
  c->mask = false;
  const bool takes = k >= K_QUANTILE;
  if (takes != (col != std::string::npos)) return false;
  if (!takes) return true;
  const std::string rest = t.substr(col + 1);
  if (k == K_OUTLIERS) {
    if (rest != "0" && rest != "1") return false;
    c->mask = rest == "1";
    return true;
  }
  size_t at = 0;
  while (at <= rest.size()) {
    size_t end = rest.find(',', at);
    if (end == std::string::npos) end = rest.size();
    if (c->np >= BLDP_MAX_QUANTILES || end == at) return false;
    c->p[c->np++] = strtod(rest.substr(at, end - at).c_str(), nullptr);
    at = end + 1;
  }
  return k == K_QUANTILES ? c->np >= 1 : c->np == 1;
}

// ---- --reach ----------------------------------------------------------------
struct Reach {
  int64_t elems = -1;
  std::string at;
};
std::map<const void *, Reach> g_reach;

void reach_case(const Case &c, uint64_t *cases, uint64_t *errors) {
  int64_t plan[10];
  ++*cases;
  if (!run_call(c, plan)) {
    ++*errors;
    fprintf(stderr, "refused: %s\n", case_line(c).c_str());
    return;
  }
  const int64_t elems = c.nchan * c.nif * c.ntime;
  for (const Launch &l : g_launches) {
    Reach &r = g_reach[l.fn];
    if (r.elems >= 0 && r.elems <= elems) continue;
    r.elems = elems;
    r.at = case_line(c);
  }
}

// Block lengths: both sides of plan_stats' switches (the lanes of k_mom_lanes
// and k_median_sort: powers of two of values or float4s to 64 lanes; kSortMaxF
// 64, kLaneMaxF 1024, kRegMaxF 4096) with and without float4 items ...
const int64_t kF[] = {1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 20, 32, 33, 36, 64, 65, 68, 128, 129, 132,
                      256, 257, 260, 512, 513, 516, 1024, 1025, 1028, 4096, 4097, 4100};
// ... and of plan_tstat's and launch_tstat's (the register forms' 2 .. 32,
// kRegMaxT 32, kChunkMin 4096: a chunk count of 2 from 8192)
const int64_t kT[] = {2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 4096, 8192};
// Channels of a time-block window: with and without float4 columns, below and
// above a split tile (32 columns, 16 for quantiles of two or more lower
// ranks), few enough for plan_tstat to cut time chunks and many enough for it
// to keep the widest tile
const int64_t kNcT[] = {1, 2, 3, 4, 5, 8, 12, 15, 16, 17, 20, 31, 32, 33, 36, 64, 68, 128, 132,
                        1024, 1028, 16384};
// The window in its array: the channel step (1, 2, -1) and a start 3 floats in
struct WinKind {
  int step, off;
};
const WinKind kWin[] = {{1, 0}, {1, 3}, {2, 0}, {2, 3}, {-1, 0}, {-1, 3}};

Case make_case(const WinKind &wk, int axis, int64_t n, int64_t nc, int64_t ni, int64_t nt,
               int nbank, bool words) {
  Case c{};
  c.axis = axis, c.n = n, c.nbank = nbank, c.words = words;
  c.nif = ni, c.ntime = nt;
  const int64_t span = wk.step == 2 ? 2 * nc - 1 : nc;
  c.nchan = span + wk.off;
  c.has_win = !(wk.step == 1 && wk.off == 0);
  const int64_t start = wk.step < 0 ? wk.off + nc - 1 : wk.off;
  const int64_t w[9] = {start, nc, wk.step, 0, ni, 1, 0, nt, 1};
  memcpy(c.win, w, sizeof w);
  return c;
}

// The ops of the sweep for blocks of n: the four plain ones; quantile at both
// clamps and inside; quantiles with L = 1 .. min(8, n - 1) distinct lower ranks,
// spread over the block (2 L ranks where no two are neighbours) and adjacent
// (L + 1 ranks); outliers with and without a mask.
std::vector<Case> with_ops(const Case &base) {
  std::vector<Case> v;
  const int64_t n = base.n;
  for (OpKind k : {K_VAR, K_STD, K_MEDIAN, K_MAD}) {
    Case c = base;
    c.kind = k;
    v.push_back(c);
  }
  for (double p : {0.0, 0.3, 1.0}) {
    Case c = base;
    c.kind = K_QUANTILE, c.np = 1, c.p[0] = p;
    v.push_back(c);
  }
  if (n >= 2) {
    for (int L = 1; L <= BLDP_MAX_QUANTILES && L <= n - 1; ++L)
      for (int spread = 0; spread < 2; ++spread) {
        Case c = base;
        c.kind = K_QUANTILES, c.np = L;
        for (int k = 0; k < L; ++k) {  // lower rank r: p = (r + 1/2) / (n - 1)
          const int64_t r = spread ? k * (n - 1) / L : k;
          c.p[k] = ((double)r + 0.5) / (double)(n - 1);
        }
        v.push_back(c);
      }
    for (int m = 0; m < 2; ++m) {
      Case c = base;
      c.kind = K_OUTLIERS, c.mask = m != 0;
      v.push_back(c);
    }
  }
  return v;
}

int reach() {
  uint64_t cases = 0, errors = 0;
  for (int words = 1; words >= 0; --words)  // (aligned first: the smallest input named is one)
    for (const WinKind &wk : kWin)
      for (int64_t ni = 1; ni <= 2; ++ni)
        for (int nbank = 1; nbank <= 2; ++nbank) {
          for (int64_t F : kF)
            for (int64_t nco : {1, 2, 5})
              for (int64_t nt : {1, 2})
                for (const Case &c : with_ops(make_case(wk, 0, F, F * nco, ni, nt, nbank, words != 0)))
                  reach_case(c, &cases, &errors);
          for (int64_t T : kT)
            for (int64_t nc : kNcT)
              for (int64_t nb : {1, 2, 3})
                for (const Case &c : with_ops(make_case(wk, 2, T, nc, ni, T * nb, nbank, words != 0)))
                  reach_case(c, &cases, &errors);
        }
  for (const auto &kv : g_reach)
    printf("reach sym=%s elems=%lld case=%s\n", sym_of(kv.first), (long long)kv.second.elems,
           kv.second.at.c_str());
  printf("total cases=%llu errors=%llu\n", (unsigned long long)cases, (unsigned long long)errors);
  return errors ? 1 : 0;
}

int list_symbols() {
  for (const auto &kv : names())
    if (is_stat_symbol(kv.second)) printf("%s\n", kv.second.c_str());
  return 0;
}

int run_cases() {
  static char line[1 << 16];
  uint64_t n = 0, errors = 0;
  while (fgets(line, sizeof line, stdin)) {
    std::vector<std::string> tok;
    for (char *t = strtok(line, " \t\r\n"); t; t = strtok(nullptr, " \t\r\n")) tok.push_back(t);
    if (tok.empty() || tok[0][0] == '#') continue;
    ++n;
    printf("case");
    for (const std::string &t : tok) printf(" %s", t.c_str());
    bool ok = tok.size() == 9;
    Case c{};
    if (ok && tok[3] != "-") {
      long long w[9];
      c.has_win = sscanf(tok[3].c_str(), "%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld", &w[0],
                         &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8]) == 9;
      for (int q = 0; q < 9; ++q) c.win[q] = w[q];
      ok = c.has_win;
    }
    int64_t plan[10] = {};
    if (ok) {
      c.nchan = atoll(tok[0].c_str()), c.nif = atoll(tok[1].c_str()), c.ntime = atoll(tok[2].c_str());
      c.axis = atoi(tok[4].c_str()), c.n = atoll(tok[5].c_str());
      c.nbank = atoi(tok[6].c_str()), c.words = atoi(tok[7].c_str()) != 0;
      ok = parse_op(tok[8], &c) && run_call(c, plan);
    }
    if (ok) {
      printf(" | rc=0 plan=");
      for (int q = 0; q < 10; ++q) printf("%s%lld", q ? "," : "", (long long)plan[q]);
      for (const Launch &l : g_launches)
        printf(" | launch sym=%s gx=%u gy=%u gz=%u bx=%u by=%u bz=%u", sym_of(l.fn), l.grid.x,
               l.grid.y, l.grid.z, l.block.x, l.block.y, l.block.z);
    } else {
      ++errors;
      printf(" | rc=1");
    }
    printf("\n");
  }
  printf("total cases=%llu errors=%llu\n", (unsigned long long)n, (unsigned long long)errors);
  return errors ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "--list")) return list_symbols();
  if (argc == 2 && !strcmp(argv[1], "--cases")) return run_cases();
  if (argc == 2 && !strcmp(argv[1], "--reach")) return reach();
  fprintf(stderr, "usage: %s --list | --reach | --cases\n", argv[0]);
  return 2;
}
