// reduce_launch_record — what the Float32 reduce's planner and dispatcher do,
// recorded on the host: the host half of kernels.hip linked into this program,
// which stands in for the few HIP runtime entry points that half calls.  It
// calls plan_reduce and launch_reduce over a sweep of shapes, alignments and
// plan options and prints, per case, the plan and every launch: the kernel
// symbol, the grid, the block, the dynamic LDS bytes and the RedArgs the
// launch received, field by field.  The device code the objects would register
// is absent: its __hip_fatbin_* symbols are defined as 0 at link time.  It
// needs no GPU and no HIP runtime library and is never loaded into Python
// (tests/test_reduce_dispatch_host.py builds and runs it).  From the
// repository root:
//
//   mkdir -p build/rlr && /opt/rocm/bin/hipcc --cuda-host-only -O1 -std=c++17 -Iinclude -DBLDP_BUILD -c bldistributeddataproducts.jl_amd/csrc/kernels.hip -o build/rlr/kernels.o && /opt/rocm/bin/hipcc --cuda-host-only -O1 -std=c++17 -Iinclude -Ibldistributeddataproducts.jl_amd/csrc -DBLDP_BUILD -x hip -c tools/reduce_launch_record.cpp -o build/rlr/record.o && /opt/rocm/lib/llvm/bin/clang++ build/rlr/record.o build/rlr/kernels.o $(/opt/rocm/lib/llvm/bin/llvm-readelf --syms build/rlr/kernels.o build/rlr/record.o | grep -o '__hip_fatbin_[0-9a-f]*' | sort -u | sed 's/.*/-Wl,--defsym=&=0/') -o build/rlr/reduce_launch_record && build/rlr/reduce_launch_record 11 67 | tail -n 1
//
// Usage: reduce_launch_record SHAPE_STRIDE OPTION_STRIDE   the sweep: every
//          SHAPE_STRIDE-th shape at the default plan, every OPTION_STRIDE-th
//          under each plan option value (1 1: the full cross product)
//        reduce_launch_record --loop N   the host cost of N dispatches of the
//          prepared cfg4 band reduce (bench.py), in ns per launch_reduce
//        reduce_launch_record --reach SHAPE_STRIDE OPTION_STRIDE   the same sweep,
//          with all four ops per case, printing only, per symbol started, the
//          smallest input (elements per bank) that started it
//        reduce_launch_record --list   every registered k_reduce_* entry point
//        reduce_launch_record --cases   what each case read from stdin runs, one
//          case per line:
//            NCHAN NIF NTIME WINDOW F T OP NBANK STITCHED [OPTION:VALUE ...]
//          WINDOW is - or nine comma-separated integers (start, count, step of
//          the channel, IF and time axes, 0-based, as bldp_reduce_f32 takes
//          them).  RedArgs and the alignment classes are formed as
//          prepare_reduce (api.hip) forms them, for 16-byte aligned banks and
//          output, on 256 CUs at XCD order lg 3.  Printed per case: plan=, the
//          fields bldp_reduce_plan_f32 reports of that launch (path, lanes per
//          group, time-split waves, float4 per lane, time chunks, workgroups,
//          vec_out); query=, the same of one bank of the case reduced alone
//          into a dense array (what bldp_reduce_plan_f32, which takes one
//          bank, answers); and the symbols launched.
#include <cxxabi.h>

#include <chrono>
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
  size_t shm;
  bldp::RedArgs args;
};
std::vector<Launch> g_launches;
bool g_record = true;
uint64_t g_count = 0;

std::map<const void *, std::string> &names() {
  static std::map<const void *, std::string> m;  // (filled by static constructors)
  return m;
}

// "void bldp::(anonymous namespace)::k_reduce_rowt<0, 1, 4, 8, false>(bldp::RedArgs)"
// -> "k_reduce_rowt<0,1,4,8,false>"
std::string short_name(const char *mangled) {
  int st = 0;
  char *d = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
  std::string s = st == 0 && d ? d : mangled;
  free(d);
  const size_t k = s.find("k_");
  if (k != std::string::npos) s = s.substr(k);
  const size_t par = s.rfind('(');
  if (par != std::string::npos) s = s.substr(0, par);
  std::string o;
  for (char c : s)
    if (c != ' ') o += c;
  return o;
}

hipError_t record(const void *fn, dim3 grid, dim3 block, void **args, size_t shm) {
  ++g_count;
  if (!g_record) return hipSuccess;
  Launch l{fn, grid, block, shm, *static_cast<const bldp::RedArgs *>(args[0])};
  g_launches.push_back(l);
  return hipSuccess;
}

struct CallConfig {
  dim3 grid, block;
  size_t shm;
  hipStream_t stream;
};
thread_local CallConfig t_cfg;

}  // namespace

// The runtime entry points the host half of kernels.hip calls.
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
hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t shm,
                           hipStream_t) {
  return record(fn, grid, block, args, shm);
}
hipError_t hipExtLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t shm,
                              hipStream_t, hipEvent_t, hipEvent_t, int) {
  return record(fn, grid, block, args, shm);
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

using bldp::Plan;
using bldp::RedArgs;

// the plan's kernel, by the name its k_reduce_* entry carries
const char *const kKernelNames[] = {"vec",    "wavet",   "il",         "row",  "rows",
                                    "rowt",   "narrow",  "narrowt",    "narrow_mis", "lane",
                                    "lanet",  "lanes",   "col3",       "tile", "scalar"};
static_assert(sizeof(kKernelNames) / sizeof(kKernelNames[0]) == bldp::RK_COUNT,
              "one name per ReduceKernel");
const char *plan_kernel(const Plan &p) { return kKernelNames[p.kernel]; }

struct Align {
  bool aligned, rows16, words;
  int cs;
};
// (aligned, rows16, words) as prepare_reduce can form them: 16-byte columns;
// dword-aligned unit-step windows taken as vectors (unaligned_vec); a
// misaligned start on 16-byte rows; odd pitches; pointers off a dword; and
// the two of a channel step of 2
const Align kAligns[] = {{true, true, true, 1},   {true, false, true, 1}, {false, true, true, 1},
                         {false, false, true, 1}, {false, false, false, 1},
                         {false, true, false, 2}, {false, false, false, 2}};
struct Banks {
  int nbank;
  bool stitched;
};
const Banks kBanks[] = {{1, true}, {1, false}, {8, true}, {8, false}};
// (every value of kRowG4, kIlK4, kLaneF, kLanetF and every (kVecLpg, VecK4c)
// pair occurs: 32, 128 for G4 = 8, 32; 2048 for K4 = 8; 24 .. 768 for K4C = 3
// and 20 .. 640 for the generic K4C = 0 at each LPG)
const int64_t kF[] = {1,   2,   3,   4,   5,   6,   7,   8,   12,   16,   20,
                      24,  32,  40,  48,  64,  80,  96,  128, 160,  192,  256,
                      320, 384, 512, 640, 768, 1024, 2048, 4096, 65536};
const int64_t kT[] = {1, 2, 3, 4, 8, 16, 272, 1024};
// (256 and 2048: banks of 1 .. 16 groups, which k_reduce_rowt and k_reduce_wavet
// pack; 840 and 65520: rows that groups of 5 and of 12 channels divide, 840 in
// fewer than 241 groups of 5, k_reduce_lanes' limit; 15 * 2^20: those of
// 3 * 2^k and 5 * 2^k channels)
const int64_t kRows[] = {16, 42, 256, 512, 840, 2048, 4096, 65520, 65536, (int64_t)15 << 20, (int64_t)1 << 26};
const int64_t kNto[] = {1, 2, 17, 100000};
const int64_t kNi[] = {1, 2};
const int kXcd[] = {0, 3};
constexpr int kNumCus = 256;

struct OptVal {
  const char *name;
  int64_t v;
};
// every reduce plan option at every value tests/test_gpu_parity.py's
// test_plan_options_every_form uses
const OptVal kOpts[] = {
    {"row_split", 1}, {"row_split", 2}, {"row_split", 4}, {"ts_fill", 0}, {"ts_fill", 1},
    {"narrow_mis", 0}, {"narrow_mis", 1}, {"t38", 0}, {"t38", 1}, {"wide_split", 0},
    {"wide_split", 1}, {"narrow_tpb", 0}, {"narrow_tpb", 1}, {"narrow_tpb", 2}, {"lane", 0},
    {"lane", 1}, {"lane3", 0}, {"lane3", 1}, {"lanet", 0}, {"lanet", 1}, {"lanet_pack", 0},
    {"lanet_pack", 1}, {"vec_il", 0}, {"vec_il", 1}, {"vec_row", 0}, {"vec_row", 1},
    {"row_tpb", 0}, {"row_tpb", 1}, {"rowt_pack", 0}, {"rowt_pack", 1}, {"rowt_small", 0},
    {"rowt_small", 64}, {"rowt_small", 100000}, {"wavet", 0}, {"wavet", 1},
    {"unaligned_vec", 0}, {"unaligned_vec", 1}, {"unaligned_vec", 2}, {"row_bpack", 0},
    {"row_bpack", 1}, {"lane_bpack", 0}, {"lane_bpack", 1}, {"wave_bpack", 0}, {"wave_bpack", 1},
    {"col3", 0}, {"col3", 1}, {"rowt_narrow8", 0}, {"rowt_narrow8", 1}, {"st_plain", 0},
    {"st_plain", 1}, {"st_plain", 2}};

const float *fake_in(int b) { return (const float *)(uintptr_t)(0x100000000ull + 0x10000000ull * b); }

// The RedArgs prepare_reduce (api.hip) would hand the planner.
RedArgs make_args(int64_t F, int64_t T, int64_t rows, int64_t nto, int64_t ni, Banks bk,
                  Align al) {
  RedArgs a{};
  a.nco = rows / F;
  a.ni = ni;
  a.nto = nto;
  a.F = F;
  a.T = T;
  a.nbank = bk.nbank;
  float *out = (float *)(uintptr_t)0x7000000000ull;
  if (bk.stitched) {
    a.out_bank = a.nco;
    a.out_ld_i = bk.nbank * a.nco;
    a.out_ld_t = bk.nbank * a.nco * ni;
  } else {  // dense per bank, one float off a 16-byte boundary
    a.out_bank = a.nco * ni * nto;
    a.out_ld_i = a.nco;
    a.out_ld_t = a.nco * ni;
    out += 1;
  }
  a.out = out;
  const int64_t pitch = rows * al.cs + (al.rows16 ? 0 : 1);
  a.in_off = al.aligned && al.rows16 ? 0 : 1;
  a.in_cs = al.cs;
  a.in_ld_i = pitch;
  a.in_ld_t = pitch * ni;
  for (int b = 0; b < bk.nbank; ++b) a.in[b] = fake_in(b);
  return a;
}

void print_args(const RedArgs &a) {
  printf(" out=%llx ws=%llx out_bank=%lld out_ld_i=%lld out_ld_t=%lld in_off=%lld in_cs=%lld "
         "in_ld_i=%lld in_ld_t=%lld nco=%lld ni=%lld nto=%lld F=%lld T=%lld rows_per_chunk=%lld "
         "blocks_c=%lld ntiles=%lld nchunk=%d nbank=%d ts=%d k4=%d vec_out=%d gpt=%lld tpb=%d "
         "tsub_log2=%d bpack=%d rsplit=%d st_plain=%d xcd_lg=%d div=%g",
         (unsigned long long)(uintptr_t)a.out, (unsigned long long)(uintptr_t)a.ws,
         (long long)a.out_bank, (long long)a.out_ld_i, (long long)a.out_ld_t, (long long)a.in_off,
         (long long)a.in_cs, (long long)a.in_ld_i, (long long)a.in_ld_t, (long long)a.nco,
         (long long)a.ni, (long long)a.nto, (long long)a.F, (long long)a.T,
         (long long)a.rows_per_chunk, (long long)a.blocks_c, (long long)a.ntiles, a.nchunk,
         a.nbank, a.ts, a.k4, a.vec_out, (long long)a.gpt, a.tpb, a.tsub_log2, a.bpack, a.rsplit,
         a.st_plain, a.xcd_lg, (double)a.div);
}

struct Reach {
  int64_t elems = -1;
  std::string at;
};
bool g_reach = false;
std::map<std::string, Reach> &reach() {
  static std::map<std::string, Reach> m;
  return m;
}

// One case: plan, launch, print.  Returns whether launch_reduce succeeded.
bool run_case(uint64_t idx, int64_t F, int64_t T, int64_t rows, int64_t nto, int64_t ni, Banks bk,
              Align al, int xcd_lg, const char *optname, int64_t optval) {
  RedArgs a = make_args(F, T, rows, nto, ni, bk, al);
  const Plan p = bldp::plan_reduce(a, al.aligned, al.rows16, al.words, kNumCus, xcd_lg);
  if (p.ws_bytes) a.ws = (float *)(uintptr_t)0x6000000000ull;
  const int op = (int)(idx % 4);  // sum, mean, max, min
  g_launches.clear();
  const hipError_t e = bldp::launch_reduce(a, p, op, nullptr);
  if (g_reach) {  // --reach: the smallest input (elements per bank) that started each symbol
    bool ok = e == hipSuccess;  // (of all four ops: g_launches collects them)
    for (int o = 1; o < 4; ++o) ok = bldp::launch_reduce(a, p, (op + o) % 4, nullptr) == hipSuccess && ok;
    const int64_t elems = (rows * al.cs + (al.rows16 ? 0 : 1)) * ni * nto * T;
    for (const Launch &l : g_launches) {
      const auto it = names().find(l.fn);
      Reach &r = reach()[it == names().end() ? "?" : it->second];
      if (r.elems >= 0 && r.elems <= elems) continue;
      char buf[256];
      snprintf(buf, sizeof buf,
               "F=%lld T=%lld rows=%lld nto=%lld ni=%lld nbank=%d stitched=%d aligned=%d "
               "rows16=%d words=%d cs=%d xcd=%d opt=%s:%lld",
               (long long)F, (long long)T, (long long)rows, (long long)nto, (long long)ni,
               bk.nbank, (int)bk.stitched, (int)al.aligned, (int)al.rows16, (int)al.words, al.cs,
               xcd_lg, optname, (long long)optval);
      r.elems = elems;
      r.at = buf;
    }
    return ok;
  }
  printf("case F=%lld T=%lld rows=%lld nto=%lld ni=%lld nbank=%d stitched=%d aligned=%d rows16=%d "
         "words=%d cs=%d xcd=%d opt=%s:%lld op=%d | rc=%d path=%d kernel=%s lpg=%d grid=%lld "
         "nout=%lld ws_bytes=%llu nlaunch=%zu",
         (long long)F, (long long)T, (long long)rows, (long long)nto, (long long)ni, bk.nbank,
         (int)bk.stitched, (int)al.aligned, (int)al.rows16, (int)al.words, al.cs, xcd_lg, optname,
         (long long)optval, op, (int)e, p.path, plan_kernel(p), p.lpg, (long long)p.grid,
         (long long)p.nout, (unsigned long long)p.ws_bytes, g_launches.size());
  for (size_t k = 0; k < g_launches.size(); ++k) {
    const Launch &l = g_launches[k];
    const auto it = names().find(l.fn);
    printf(" | launch sym=%s gx=%u gy=%u gz=%u bx=%u by=%u bz=%u shm=%zu",
           it == names().end() ? "?" : it->second.c_str(), l.grid.x, l.grid.y, l.grid.z,
           l.block.x, l.block.y, l.block.z, l.shm);
    if (k == 0) print_args(l.args);
  }
  printf("\n");
  return e == hipSuccess;
}

// The shapes under one option setting, every stride-th of them.
void sweep(uint64_t stride, const char *optname, int64_t optval, uint64_t *cases, uint64_t *errors) {
  uint64_t idx = 0;
  for (int64_t F : kF)
    for (int64_t T : kT)
      for (int64_t rows : kRows) {
        if (rows % F) continue;
        for (int64_t nto : kNto)
          for (int64_t ni : kNi)
            for (Banks bk : kBanks)
              for (Align al : kAligns)
                for (int xcd : kXcd) {
                  if (idx++ % stride) continue;
                  ++*cases;
                  if (!run_case(idx, F, T, rows, nto, ni, bk, al, xcd, optname, optval)) ++*errors;
                }
      }
}

int loop(long n) {
  // cfg4 (bench.py): 8 banks of 512 channels x 1 IF, 879616 spectra, F = 8, T = 1024
  RedArgs a = make_args(8, 1024, 512, 859, 1, Banks{8, true}, kAligns[0]);
  const Plan p = bldp::plan_reduce(a, true, true, true, kNumCus, 3);
  if (p.ws_bytes) a.ws = (float *)(uintptr_t)0x6000000000ull;
  g_record = false;
  double best = 1e30;
  for (int rep = 0; rep < 9; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long k = 0; k < n; ++k)
      if (bldp::launch_reduce(a, p, 0, nullptr) != hipSuccess) return 1;
    const double ns =
        std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n;
    printf("rep %d: %.2f ns per launch_reduce\n", rep, ns);
    if (ns < best) best = ns;
  }
  printf("best of 9: %.2f ns per launch_reduce (%llu stub launches)\n", best,
         (unsigned long long)g_count);
  return 0;
}

// --cases: api.hip's resolve_window, resolve_factors and prepare_reduce, restated.
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
bool unaligned_vec_pays(int64_t F, bool rows16) {
  if (!rows16) return true;
  return F == 1 || (F % 4 == 0 && F <= 256);
}

struct Public {  // bldp_reduce_plan_f32's info[0..5], info[7]
  int64_t v[7];
};
Public public_plan(const RedArgs &a, const Plan &p) {
  return Public{{p.path, p.lpg, p.path == bldp::PATH_VEC_ROW ? a.rsplit : a.ts, a.k4, a.nchunk,
                 p.grid, a.vec_out}};
}
void print_public(const char *key, const Public &q) {
  printf(" %s=%lld,%lld,%lld,%lld,%lld,%lld,%lld", key, (long long)q.v[0], (long long)q.v[1],
         (long long)q.v[2], (long long)q.v[3], (long long)q.v[4], (long long)q.v[5],
         (long long)q.v[6]);
}

// The RedArgs and plan of prepare_reduce for nbank 16-byte aligned banks and a
// 16-byte aligned output: stitched, or dense per bank (bldp_reduce_f32).
bool prepare_case(int nbank, bool stitched, int64_t nchan, int64_t nif, int64_t ntime,
                  const int64_t *win, int64_t fqavby, int64_t tavby, RedArgs *ap, Plan *pp) {
  if (nbank < 1 || nbank > BLDP_MAX_BANKS) return false;
  Geo g;
  if (!resolve_window(nchan, nif, ntime, win, &g)) return false;
  const int64_t F = fqavby <= 1 ? 1 : fqavby, T = tavby <= 1 ? 1 : tavby;
  if (g.nc % F != 0 || g.nt % T != 0) return false;
  RedArgs &a = *ap;
  a = RedArgs{};
  a.nco = g.nc / F;
  a.ni = g.ni;
  a.nto = g.nt / T;
  a.F = F;
  a.T = T;
  a.nbank = nbank;
  if (stitched) {
    a.out_bank = a.nco;
    a.out_ld_i = nbank * a.nco;
    a.out_ld_t = nbank * a.nco * a.ni;
  } else {
    a.out_bank = a.nco * a.ni * a.nto;
    a.out_ld_i = a.nco;
    a.out_ld_t = a.nco * a.ni;
  }
  a.in_off = g.off;
  a.in_cs = g.cs;
  a.in_ld_i = g.ld_i;
  a.in_ld_t = g.ld_t;
  a.out = (float *)(uintptr_t)0x7000000000ull;
  if (a.nco == 0 || a.ni == 0 || a.nto == 0) return false;  // (nothing is launched)
  const bool rows16 = pitch_ok(g), words = true;  // (the banks: 16-byte aligned)
  for (int b = 0; b < nbank; ++b) a.in[b] = fake_in(b);
  const bool aligned = (rows16 && vec_ok(g)) ||
                       (bldp::opt(bldp::OPT_UNALIGNED_VEC) >= 1 && words && g.cs == 1 &&
                        unaligned_vec_pays(F, rows16));
  *pp = bldp::plan_reduce(a, aligned, rows16, words && g.cs == 1, kNumCus, 3);
  return true;
}

int list_symbols() {
  for (const auto &kv : names())
    if (kv.second.rfind("k_reduce_", 0) == 0) printf("%s\n", kv.second.c_str());
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
    bool ok = tok.size() >= 9;
    int64_t win[9];
    bool has_win = false;
    if (ok && tok[3] != "-") {
      has_win = sscanf(tok[3].c_str(), "%ld,%ld,%ld,%ld,%ld,%ld,%ld,%ld,%ld", &win[0], &win[1],
                       &win[2], &win[3], &win[4], &win[5], &win[6], &win[7], &win[8]) == 9;
      ok = has_win;
    }
    std::vector<int> set;
    for (size_t k = 9; ok && k < tok.size(); ++k) {
      const size_t c = tok[k].find(':');
      const int o = c == std::string::npos ? -1 : bldp::plan_opt_index(tok[k].substr(0, c).c_str());
      const int64_t v = c == std::string::npos ? -1 : atoll(tok[k].c_str() + c + 1);
      if (o < 0 || v < 0 || !bldp::plan_opt_valid(o, v)) {
        ok = false;
        break;
      }
      bldp::plan_opt_set(o, v);
      set.push_back(o);
    }
    if (ok) {
      const int64_t nchan = atoll(tok[0].c_str()), nif = atoll(tok[1].c_str()),
                    ntime = atoll(tok[2].c_str()), F = atoll(tok[4].c_str()),
                    T = atoll(tok[5].c_str());
      const int op = atoi(tok[6].c_str()), nbank = atoi(tok[7].c_str());
      const bool stitched = atoi(tok[8].c_str()) != 0;
      RedArgs a, a1;
      Plan p, p1;
      ok = op >= 0 && op <= 3 &&
           prepare_case(nbank, stitched, nchan, nif, ntime, has_win ? win : nullptr, F, T, &a, &p) &&
           prepare_case(1, false, nchan, nif, ntime, has_win ? win : nullptr, F, T, &a1, &p1);
      if (ok) {
        if (p.ws_bytes) a.ws = (float *)(uintptr_t)0x6000000000ull;
        g_launches.clear();
        ok = bldp::launch_reduce(a, p, op, nullptr) == hipSuccess && !g_launches.empty();
      }
      if (ok) {
        printf(" | rc=0 kernel=%s", plan_kernel(p));
        print_public("plan", public_plan(a, p));
        print_public("query", public_plan(a1, p1));
        for (const Launch &l : g_launches) {
          const auto it = names().find(l.fn);
          printf(" | launch sym=%s", it == names().end() ? "?" : it->second.c_str());
        }
      }
    }
    for (int o : set) bldp::plan_opt_set(o, -1);
    if (!ok) {
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
  if (argc == 3 && !strcmp(argv[1], "--loop")) return loop(atol(argv[2]));
  if (argc == 4 && !strcmp(argv[1], "--reach")) g_reach = true, ++argv, --argc;
  if (argc != 3 || atol(argv[1]) < 1 || atol(argv[2]) < 1) {
    fprintf(stderr, "usage: %s [--reach] SHAPE_STRIDE OPTION_STRIDE | --loop N | --list | --cases\n", argv[0]);
    return 2;
  }
  uint64_t cases = 0, errors = 0;
  sweep((uint64_t)atol(argv[1]), "default", -1, &cases, &errors);
  for (const OptVal &o : kOpts) {
    const int k = bldp::plan_opt_index(o.name);
    if (k < 0) {
      fprintf(stderr, "unknown plan option %s\n", o.name);
      return 2;
    }
    bldp::plan_opt_set(k, o.v);
    sweep((uint64_t)atol(argv[2]), o.name, o.v, &cases, &errors);
    bldp::plan_opt_set(k, -1);
  }
  for (const auto &kv : reach())
    printf("reach sym=%s elems=%lld %s\n", kv.first.c_str(), (long long)kv.second.elems,
           kv.second.at.c_str());
  printf("total cases=%llu errors=%llu\n", (unsigned long long)cases, (unsigned long long)errors);
  return errors ? 1 : 0;
}
