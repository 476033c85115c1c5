// kurt_launch_record — what the time-moment family's planner and dispatcher do
// (getkurtosis, getskewness, getmoments, over the whole window and over blocks
// of spectra), recorded on the host: the host half of kurtosis.hip linked into
// this program, which stands in for the few HIP runtime entry points that half
// calls.  kernels.hip's host half comes along for the plan options.  The device
// code the objects would register is absent: its __hip_fatbin_* symbols are
// defined as 0 at link time.  It needs no GPU and no HIP runtime library and
// is never loaded into Python.  tests/test_kurt_reach_host.py's `tool` fixture
// is the build recipe (three --cuda-host-only compiles and one link that
// defines every __hip_fatbin_* symbol of the objects as 0) and runs it.
//
// KurtArgs / KurtBlkArgs are formed by the rules of kurt_setup, mom_plan and
// mom_run (api.hip), restated here: rows16 / vec (plan option unaligned_vec),
// the one-launch block form, the block-by-block form, and results written in
// place (`direct`) or staged and scattered.  The banks are taken as 16-byte
// aligned (what torch's allocations are; a window's own channel start and the
// array's pitches decide the rest), on 256 CUs.
//
// Usage: kurt_launch_record --list    every registered entry point of
//          kurtosis.hip (k_kurt*, k_fill_nan), one per line
//        kurt_launch_record --reach   a sweep over spectrum counts on both sides
//          of every switch of launch_kurtosis, with_regs_form, launch_tree,
//          launch_final and launch_kurt_blocks; channel counts and steps with
//          and without float4 columns; 1-3 IFs and banks; tblock 0, <= 32,
//          33..1024 and > 1024; orders 4, 3 and kOrdAll (0); and every value of
//          the plan options kurt_exact, kurt_mid_cpl, kurt_mid_small,
//          kurt_leaf_narrow, kurt_leaf_tile and unaligned_vec.  Prints, per
//          entry point started, the smallest input (elements per bank) that
//          started it, as a line --cases takes
//        kurt_launch_record --cases   what each case read from stdin runs, one
//          case per line, as the API takes it:
//            NCHAN NIF NTIME WINDOW ORDER TBLOCK NBANK DENSE [OPTION:VALUE ...]
//          WINDOW is - or nine comma-separated integers (start, count, step of
//          the channel, IF and time axes, 0-based).  ORDER is 4, 3 or 0
//          (kOrdAll).  TBLOCK 0 is the whole window; ORDER 4 TBLOCK 0 is
//          bldp_kurtosis_f32 / bldp_band_kurtosis_f32, every other pair
//          bldp_{kurtosis_blocks,skewness,moments}_f32 or its band entry.
//          DENSE 1 is the dense result those take from the engine (the band
//          entries for NBANK > 1); DENSE 0 (NBANK 1, not ORDER 4 TBLOCK 0) a
//          strided one, out_ld_i = nc + 3 and out_ld_b = ni out_ld_i + 5.
//          Printed per case: plan=, the four public plan words of ONE bank
//          (ORDER 4 TBLOCK 0: path, K, leaf slots, workspace bytes of
//          bldp_kurtosis_plan_f32; else path, one-launch flag, blocks,
//          workspace bytes of bldp_*_plan_f32), and every symbol launched, in
//          order, with grid and block.
#include <cxxabi.h>

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

// "void bldp::(anonymous namespace)::k_kurt_mid<16, 4>(bldp::KurtArgs)" -> "k_kurt_mid<16,4>"
std::string short_name(const char *mangled) {
  int st = 0;
  char *d = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
  std::string s = st == 0 && d ? d : mangled;
  free(d);
  const size_t k = s.find("k_");
  if (k != std::string::npos) s = s.substr(k);
  const size_t par = s.find('(');  // (the parameter list: no template argument here has one)
  if (par != std::string::npos) s = s.substr(0, par);
  std::string o;
  for (char c : s)
    if (c != ' ') o += c;
  return o;
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

// The runtime entry points the host halves of kurtosis.hip and kernels.hip call.
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
}  // namespace bldp

namespace {

using bldp::KurtArgs;
using bldp::KurtBlkArgs;
using bldp::kOrdAll;

constexpr int kNumCus = 256;
constexpr int64_t kInt32Max = 2147483647;

bool is_kurt_symbol(const std::string &s) {
  return s.rfind("k_kurt", 0) == 0 || s.rfind("k_fill_nan", 0) == 0;
}
const char *sym_of(const void *fn) {
  const auto it = names().find(fn);
  return it == names().end() ? "?" : it->second.c_str();
}

const float *fake_in(int b) { return (const float *)(uintptr_t)(0x100000000ull + 0x10000000ull * b); }
char *fake_ws() { return (char *)(uintptr_t)0x6000000000ull; }
double *fake_out(int q) { return (double *)(uintptr_t)(0x7000000000ull + 0x100000000ull * q); }

// api.hip's resolve_window, pitch_ok and vec_ok, restated.
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
bool pitch_ok(const Geo &g) {
  return (g.ni <= 1 || g.ld_i % 4 == 0) && (g.nt <= 1 || g.ld_t % 4 == 0);
}
bool vec_ok(const Geo &g) { return g.cs == 1 && g.off % 4 == 0 && pitch_ok(g); }

// kurt_setup for nbank 16-byte aligned banks.
bool kurt_setup(int nbank, int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                KurtArgs *k, int order) {
  if (nbank < 1 || nbank > BLDP_MAX_BANKS) return false;
  Geo g;
  if (!resolve_window(nchan, nif, ntime, win, &g)) return false;
  *k = KurtArgs{};
  k->order = order;
  k->nbank = nbank;
  const bool aligned = true, words = true;
  for (int b = 0; b < nbank; ++b) k->in[b] = fake_in(b);
  k->in_off = g.off;
  k->in_cs = g.cs;
  k->in_ld_i = g.ld_i;
  k->in_ld_t = g.ld_t;
  k->nc = g.nc;
  k->ni = g.ni;
  k->nt = g.nt;
  k->nrow = (int64_t)nbank * g.ni;
  k->rows16 = vec_ok(g) && g.nc % 4 == 0 && aligned;
  k->vec = bldp::opt(bldp::OPT_UNALIGNED_VEC) >= 2 ? (g.cs == 1 && g.nc % 4 == 0 && words)
                                                   : k->rows16;
  bldp::plan_kurtosis(*k, kNumCus);
  return true;
}

// kurt_run: the launches of one planned window (its workspace a fake pointer).
bool kurt_run(KurtArgs &k, double *out) {
  if (k.nc * k.nrow == 0) return true;
  if (bldp::kurtosis_max_grid(k) > kInt32Max) return false;
  k.out = out;
  return bldp::launch_kurtosis(k, fake_ws(), nullptr) == hipSuccess;
}

void kblk_window(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int64_t M,
                 int64_t b, int64_t bw[9]) {
  const int64_t full[9] = {0, nchan, 1, 0, nif, 1, 0, ntime, 1};
  for (int q = 0; q < 9; ++q) bw[q] = win ? win[q] : full[q];
  bw[6] += b * M * bw[8];
  bw[7] = M;
}

struct MomPlan {
  KurtArgs whole, blk;
  int64_t nb;
  bool fused;
  int path;
  size_t tmp_off, ws_bytes;
};
// mom_plan; whole_ok: tblock = 0 allowed (skewness, moments)
bool mom_plan(int order, int nbank, int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
              int64_t tblock, MomPlan *p) {
  const bool whole_ok = order != 4;
  if (!kurt_setup(nbank, nchan, nif, ntime, win, &p->whole, order)) return false;
  p->nb = 1;
  if (tblock > 0 || !whole_ok) {
    if (tblock < 1 || p->whole.nt % tblock != 0) return false;
    p->nb = p->whole.nt / tblock;
  }
  p->fused = tblock > 0 && bldp::kurt_blocks_fused(p->whole, tblock);
  p->tmp_off = p->ws_bytes = 0;
  if (p->fused) {
    p->path = tblock <= 32 ? 0 : 2;
    return true;
  }
  p->blk = p->whole;
  if (tblock > 0) {
    int64_t bw[9];
    kblk_window(nchan, nif, ntime, win, tblock, 0, bw);
    if (p->nb == 0) bw[6] = 0, bw[7] = 0;
    if (!kurt_setup(nbank, nchan, nif, ntime, bw, &p->blk, order)) return false;
  }
  p->path = bldp::kurtosis_path(p->blk);
  p->ws_bytes = bldp::kurtosis_ws_bytes(p->blk);
  p->tmp_off = (p->ws_bytes + 255) & ~(size_t)255;
  if (tblock > 0)
    p->ws_bytes = p->tmp_off + (order == kOrdAll ? 4 : 1) *
                                   (size_t)(p->blk.nrow * p->blk.nc) * sizeof(double);
  return true;
}

struct Case {
  int64_t nchan, nif, ntime;
  bool has_win;
  int64_t win[9];
  int order;
  int64_t tblock;
  int nbank;
  bool dense;
};

// The call of the case: its public plan words (of one bank) and, in
// g_launches, what it starts.  False: the API would refuse it, or nothing runs.
bool run_call(const Case &c, int64_t plan[4]) {
  const int64_t *win = c.has_win ? c.win : nullptr;
  g_launches.clear();
  if (c.order != 4 && c.order != 3 && c.order != kOrdAll) return false;
  if (c.tblock < 0 || (!c.dense && c.nbank != 1)) return false;
  if (c.order == 4 && c.tblock == 0) {  // bldp_kurtosis_f32 / bldp_band_kurtosis_f32
    if (!c.dense) return false;
    KurtArgs q, k;
    if (!kurt_setup(1, c.nchan, c.nif, c.ntime, win, &q, 4)) return false;
    plan[0] = bldp::kurtosis_path(q), plan[1] = q.K, plan[2] = q.nslot;
    plan[3] = (int64_t)bldp::kurtosis_ws_bytes(q);
    if (!kurt_setup(c.nbank, c.nchan, c.nif, c.ntime, win, &k, 4)) return false;
    return kurt_run(k, fake_out(0)) && !g_launches.empty();
  }
  MomPlan q, p;
  if (!mom_plan(c.order, 1, c.nchan, c.nif, c.ntime, win, c.tblock, &q)) return false;
  plan[0] = q.path, plan[1] = c.tblock == 0 || q.fused ? 1 : 0, plan[2] = q.nb;
  plan[3] = (int64_t)q.ws_bytes;
  // mom_run
  const bool all = c.order == kOrdAll;
  const int np = all ? 4 : 1;
  if (!mom_plan(c.order, c.nbank, c.nchan, c.nif, c.ntime, win, c.tblock, &p)) return false;
  const KurtArgs &w = p.whole;
  if (w.nc * w.ni * p.nb == 0) return false;
  const int64_t out_ld_i = c.dense ? w.nc : w.nc + 3;
  const int64_t out_ld_b = c.dense ? w.nc * w.ni : w.ni * out_ld_i + 5;
  const int64_t out_bank = c.dense ? w.nc * w.ni * p.nb : 0;
  if (p.fused) {
    KurtBlkArgs k{};
    for (int b = 0; b < c.nbank; ++b) k.in[b] = w.in[b];
    k.nbank = c.nbank;
    k.in_off = w.in_off;
    k.in_ld_i = w.in_ld_i;
    k.in_ld_t = w.in_ld_t;
    k.nc = w.nc;
    k.ni = w.ni;
    k.M = c.tblock;
    k.nb = p.nb;
    k.out_bank = out_bank;
    k.out_ld_i = out_ld_i;
    k.out_ld_b = out_ld_b;
    k.order = c.order;
    if (all)
      for (int q4 = 0; q4 < 4; ++q4) k.mo[q4] = fake_out(q4);
    else
      k.out = fake_out(0);
    bldp::plan_kurt_blocks(k, kNumCus);
    if (bldp::kurt_blocks_grid(k) > kInt32Max) return false;
    return bldp::launch_kurt_blocks(k, nullptr) == hipSuccess && !g_launches.empty();
  }
  const bool direct =
      out_ld_i == w.nc && (c.nbank == 1 || (c.tblock == 0 && out_bank == w.nc * w.ni));
  if (c.tblock == 0 && direct) {
    KurtArgs k = p.blk;
    for (int q4 = 0; all && q4 < 4; ++q4) k.mo[q4] = fake_out(q4);
    return kurt_run(k, all ? nullptr : fake_out(0)) && !g_launches.empty();
  }
  const int64_t n = p.blk.nrow * p.blk.nc;
  double *tmp = reinterpret_cast<double *>(fake_ws() + p.tmp_off);
  for (int64_t b = 0; b < p.nb; ++b) {
    KurtArgs k = p.blk;
    if (b > 0) {
      int64_t bw[9];
      kblk_window(c.nchan, c.nif, c.ntime, win, c.tblock, b, bw);
      if (!kurt_setup(c.nbank, c.nchan, c.nif, c.ntime, bw, &k, c.order)) return false;
      if (bldp::kurtosis_ws_bytes(k) > p.tmp_off) return false;
    }
    double *dst[4];
    for (int q4 = 0; q4 < np; ++q4) dst[q4] = direct ? fake_out(q4) + b * out_ld_b : tmp + q4 * n;
    for (int q4 = 0; all && q4 < 4; ++q4) k.mo[q4] = dst[q4];
    if (!kurt_run(k, all ? nullptr : dst[0])) return false;
    for (int q4 = 0; !direct && q4 < np; ++q4)
      if (bldp::launch_kurt_scatter(dst[q4], c.nbank, w.ni, w.nc, fake_out(q4) + b * out_ld_b,
                                    out_bank, out_ld_i, nullptr) != hipSuccess)
        return false;
  }
  return !g_launches.empty();
}

std::string case_line(const Case &c, const char *optname, int64_t optval) {
  char buf[512];
  int n = snprintf(buf, sizeof buf, "%lld %lld %lld ", (long long)c.nchan, (long long)c.nif,
                   (long long)c.ntime);
  if (c.has_win) {
    for (int q = 0; q < 9; ++q)
      n += snprintf(buf + n, sizeof buf - n, "%s%lld", q ? "," : "", (long long)c.win[q]);
  } else {
    n += snprintf(buf + n, sizeof buf - n, "-");
  }
  n += snprintf(buf + n, sizeof buf - n, " %d %lld %d %d", c.order, (long long)c.tblock, c.nbank,
                (int)c.dense);
  if (optname) snprintf(buf + n, sizeof buf - n, " %s:%lld", optname, (long long)optval);
  return buf;
}

// ---- --reach ----------------------------------------------------------------
struct Reach {
  int64_t elems = -1;
  std::string at;
};
std::map<const void *, Reach> g_reach;

struct OptVal {
  const char *name;  // nullptr: the defaults
  int64_t v;
  // which spectrum counts per window or block the option can matter at
  int64_t nt_lo, nt_hi;
};
constexpr int64_t kAny = (int64_t)1 << 62;
const OptVal kOpts[] = {
    {nullptr, -1, 0, kAny},
    {"kurt_exact", 0, 1, 32}, {"kurt_exact", 1, 1, 32},
    {"kurt_mid_cpl", 1, 33, 512}, {"kurt_mid_cpl", 2, 33, 512},
    {"kurt_mid_small", 0, 33, 64}, {"kurt_mid_small", 1, 33, 64},
    // (a threshold in waves per CU: never, one, the default, and more than any window here has)
    {"kurt_leaf_narrow", 0, 33, kAny}, {"kurt_leaf_narrow", 1, 33, kAny},
    {"kurt_leaf_narrow", 4, 33, kAny}, {"kurt_leaf_narrow", 1 << 20, 33, kAny},
    {"kurt_leaf_tile", 0, 513, kAny}, {"kurt_leaf_tile", 1, 513, kAny},
    {"unaligned_vec", 0, 0, kAny}, {"unaligned_vec", 1, 0, kAny}, {"unaligned_vec", 2, 0, kAny}};

// Spectra per window (or per block): both sides of every boundary of
// with_regs_form (16, 32), path_of (32, 512), launch_kurtosis' two switches
// (k_kurt_mid2: 64 per form up to 384; k_kurt_mid: 64 per form up to 512),
// kurt_mid_small (64), k_kurt_tile's recipe and the one-launch block form
// (1024), and of the tree's level K (2048 * 2^K, K = 0 .. 15: launch_final's
// forms to K = 6, launch_tree's passes beyond).
std::vector<int64_t> spectra() {
  std::vector<int64_t> v = {1, 2, 3, 4, 12, 15, 16, 17, 31, 32, 33, 48, 100, 1000, 1023, 1024, 1025};
  for (int64_t b = 64; b <= 512; b += 64) v.insert(v.end(), {b - 1, b, b + 1});
  for (int K = 0; K <= 15; ++K) v.insert(v.end(), {(int64_t)2048 << K, ((int64_t)2048 << K) + 1});
  return v;
}
// Channels: with float4 columns (multiples of 4) and without; one partial
// tile, several tiles with a partial last one, and rows wide enough for every
// kurt_leaf_narrow / kurt_leaf_tile decision on 256 CUs.
const int64_t kNc[] = {1, 2, 3, 4, 5, 8, 12, 36, 64, 68, 128, 132, 256, 260, 512, 900,
                       1024, 1028, 2048, 4100, 8192, 16388, 65536};
// The window in its array: whole; a start one float off (float4 columns only
// by unaligned_vec); an odd pitch; a channel step of 2.
enum WinKind { W_WHOLE, W_OFF1, W_PITCH1, W_STEP2, W_COUNT };

Case make_case(WinKind wk, int64_t nc, int64_t ni, int64_t nt, int order, int64_t tblock,
               int nbank, bool dense) {
  Case c{};
  c.nif = ni, c.ntime = nt, c.order = order, c.tblock = tblock, c.nbank = nbank, c.dense = dense;
  c.has_win = wk != W_WHOLE;
  const int64_t w[9] = {wk == W_OFF1 ? 1 : 0, nc, wk == W_STEP2 ? 2 : 1, 0, ni, 1, 0, nt, 1};
  memcpy(c.win, w, sizeof w);
  c.nchan = wk == W_OFF1 ? nc + 4 : wk == W_PITCH1 ? nc + 1 : wk == W_STEP2 ? 2 * nc : nc;
  return c;
}

void reach_case(const Case &c, const OptVal &o, uint64_t *cases, uint64_t *errors) {
  int64_t plan[4];
  ++*cases;
  if (!run_call(c, plan)) {
    ++*errors;
    fprintf(stderr, "refused: %s\n", case_line(c, o.name, o.v).c_str());
    return;
  }
  const int64_t elems = c.nchan * c.nif * c.ntime;
  for (const Launch &l : g_launches) {
    Reach &r = g_reach[l.fn];
    if (r.elems >= 0 && r.elems <= elems) continue;
    r.elems = elems;
    r.at = case_line(c, o.name, o.v);
  }
}

int reach() {
  uint64_t cases = 0, errors = 0;
  const std::vector<int64_t> nts = spectra();
  const int orders[] = {4, 3, kOrdAll};
  for (const OptVal &o : kOpts) {
    int ko = -1;
    if (o.name) {
      ko = bldp::plan_opt_index(o.name);
      if (ko < 0 || !bldp::plan_opt_valid(ko, o.v)) {
        fprintf(stderr, "unknown plan option %s:%lld\n", o.name, (long long)o.v);
        return 2;
      }
      bldp::plan_opt_set(ko, o.v);
    }
    for (int order : orders)
      for (int64_t m : nts) {  // spectra per window or block
        if (m < o.nt_lo || m > o.nt_hi) continue;
        for (int nb = 0; nb <= 3; ++nb) {  // 0: the whole window (tblock = 0), else nb blocks of m
          if (nb > 0 && m * nb > ((int64_t)1 << 27)) continue;  // (one block reaches what three do)
          const int64_t nt = nb == 0 ? m : m * nb, tblock = nb == 0 ? 0 : m;
          for (int64_t nc : kNc)
            for (int wk = 0; wk < W_COUNT; ++wk) {
              if (o.name && !strcmp(o.name, "unaligned_vec") && wk == W_WHOLE) continue;
              for (int64_t ni = 1; ni <= 3; ++ni)
                for (int nbank = 1; nbank <= 3; ++nbank)
                  for (int dense = 1; dense >= 0; --dense) {
                    if (!dense && (nbank != 1 || (order == 4 && tblock == 0))) continue;
                    reach_case(make_case((WinKind)wk, nc, ni, nt, order, tblock, nbank, dense != 0),
                               o, &cases, &errors);
                  }
            }
        }
      }
    if (ko >= 0) bldp::plan_opt_set(ko, -1);
  }
  // no spectra at all: the NaN fill (order kOrdAll: one launch per plane)
  for (int order : orders) {
    Case c = make_case(W_WHOLE, 4, 1, 8, order, 0, 1, true);
    const int64_t w[9] = {0, 4, 1, 0, 1, 1, 3, 0, 1};
    memcpy(c.win, w, sizeof w);
    c.has_win = true;
    reach_case(c, kOpts[0], &cases, &errors);
  }
  for (const auto &kv : g_reach)
    printf("reach sym=%s elems=%lld case=%s\n", sym_of(kv.first), (long long)kv.second.elems,
           kv.second.at.c_str());
  printf("total cases=%llu errors=%llu\n", (unsigned long long)cases, (unsigned long long)errors);
  return errors ? 1 : 0;
}

int list_symbols() {
  for (const auto &kv : names())
    if (is_kurt_symbol(kv.second)) printf("%s\n", kv.second.c_str());
  return 0;
}

int run_cases() {
  char line[4096];
  uint64_t n = 0, errors = 0;
  while (fgets(line, sizeof line, stdin)) {
    std::vector<std::string> tok;
    for (char *t = strtok(line, " \t\r\n"); t; t = strtok(nullptr, " \t\r\n")) tok.push_back(t);
    if (tok.empty() || tok[0][0] == '#') continue;
    ++n;
    printf("case");
    for (const std::string &t : tok) printf(" %s", t.c_str());
    bool ok = tok.size() >= 8;
    Case c{};
    if (ok && tok[3] != "-") {
      long long w[9];
      c.has_win = sscanf(tok[3].c_str(), "%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld", &w[0],
                         &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8]) == 9;
      for (int q = 0; q < 9; ++q) c.win[q] = w[q];
      ok = c.has_win;
    }
    std::vector<int> set;
    for (size_t k = 8; ok && k < tok.size(); ++k) {
      const size_t col = tok[k].find(':');
      const int o = col == std::string::npos ? -1 : bldp::plan_opt_index(tok[k].substr(0, col).c_str());
      const int64_t v = col == std::string::npos ? -1 : atoll(tok[k].c_str() + col + 1);
      if (o < 0 || v < 0 || !bldp::plan_opt_valid(o, v)) {
        ok = false;
        break;
      }
      bldp::plan_opt_set(o, v);
      set.push_back(o);
    }
    int64_t plan[4] = {0, 0, 0, 0};
    if (ok) {
      c.nchan = atoll(tok[0].c_str()), c.nif = atoll(tok[1].c_str()), c.ntime = atoll(tok[2].c_str());
      c.order = atoi(tok[4].c_str()), c.tblock = atoll(tok[5].c_str());
      c.nbank = atoi(tok[6].c_str()), c.dense = atoi(tok[7].c_str()) != 0;
      ok = run_call(c, plan);
    }
    for (int o : set) bldp::plan_opt_set(o, -1);
    if (ok) {
      printf(" | rc=0 plan=%lld,%lld,%lld,%lld", (long long)plan[0], (long long)plan[1],
             (long long)plan[2], (long long)plan[3]);
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
