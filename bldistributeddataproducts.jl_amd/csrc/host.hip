// host.hip — bldp_reduce_host_f32: the drop-in for a worker that already holds
// the window in host memory (after h5["data"][idxs...] at
// src/gbtworkerfunctions.jl:185 or dmmap[idxs...] at :174).  The window is
// streamed to the GPU in chunks of whole output time rows on the two streams
// of a pooled staging pipeline (runtime.hip; copy of chunk k+1 overlaps the
// reduce of chunk k) and the reduced rows come back into the caller's dense
// (nco, ni, nto) buffer.  Nothing is allocated per call.
#include <math.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "bldp_impl.h"

extern "C" int bldp_reduce_shape(int64_t, int64_t, int64_t, const int64_t *, int64_t, int64_t,
                                 int64_t *);
extern "C" int bldp_kurtosis_f32(const float *, int64_t, int64_t, int64_t, const int64_t *,
                                 double *, void *, void *);
extern "C" int bldp_kurtosis_blocks_shape(int64_t, int64_t, int64_t, const int64_t *, int64_t,
                                          int64_t *);
extern "C" int bldp_kurtosis_blocks_f32(const float *, int64_t, int64_t, int64_t, const int64_t *,
                                        int64_t, double *, int64_t, int64_t, void *);
extern "C" int bldp_reduce_strided_f32(const float *, int64_t, int64_t, int64_t,
                                       const int64_t *, int64_t, int64_t, int, float *, int64_t,
                                       int64_t, void *);
extern "C" int bldp_reduce_strided(int, const void *, int64_t, int64_t, int64_t, const int64_t *,
                                   int64_t, int64_t, int, void *, int64_t, int64_t, void *);
extern "C" int bldp_kurtosis(int, const void *, int64_t, int64_t, int64_t, const int64_t *,
                             double *, void *);
extern "C" int bldp_reduce_out_dtype(int, int);

namespace {

struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

#define HCHK(x)                                                             \
  do {                                                                      \
    hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess)                                                   \
      return bldp::set_error(BLDP_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

// Run `body` on an idle staging pipeline of `dev`; both of its streams are
// drained before the pipeline goes back to the pool (also after an error), so
// no copy into caller memory is pending when the entry point returns.
template <class Body>
int with_stager(int dev, Body body) {
  bldp::Stager *sg = nullptr;
  int rc = bldp::stager_acquire(dev, &sg);
  if (rc) return rc;
  {
    DevGuard guard(dev);
    rc = body(sg);
    for (int b = 0; b < 2; ++b) {
      const hipError_t e = hipStreamSynchronize(sg->st[b]);
      if (e != hipSuccess && rc == BLDP_OK)
        rc = bldp::set_error(BLDP_EHIP, "device %d: %s", dev, hipGetErrorString(e));
    }
  }
  bldp::stager_release(sg);
  return rc;
}

// Staged window rows: element (c, i, t) of the window at
// row0[c*cs' + i*ld_i + t*ld_t] (elements of esz bytes) with c counted from the
// lowest channel touched.
struct HostWin {
  int64_t nc, cs, acs, span, ni, ld_i, ld_t, esz;
  const char *row0;
  bool uniform;   // rows are a single 2-D copy
  int64_t pitch;  // of that copy, in elements
};

HostWin host_window(const void *in, int64_t esz, int64_t nchan, int64_t nif, const int64_t *win,
                    int64_t nc, int64_t ni) {
  HostWin h;
  h.esz = esz;
  const int64_t c0 = win ? win[0] : 0, cs = win ? win[2] : 1;
  const int64_t i0 = win ? win[3] : 0, is = win ? win[5] : 1;
  const int64_t t0 = win ? win[6] : 0, ts = win ? win[8] : 1;
  h.nc = nc;
  h.ni = ni;
  h.cs = cs;
  h.acs = cs < 0 ? -cs : cs;
  h.span = (nc - 1) * h.acs + 1;                        // staged floats per (i, t) row
  const int64_t c_lo = cs < 0 ? c0 + (nc - 1) * cs : c0;  // lowest channel touched
  h.ld_i = nchan * is;
  h.ld_t = nchan * nif * ts;
  h.row0 = static_cast<const char *>(in) + (c_lo + nchan * (i0 + nif * t0)) * esz;
  h.uniform = (ni == 1 && h.ld_t > 0 && h.ld_t >= h.span) ||
              (h.ld_i > 0 && h.ld_i >= h.span && h.ld_t == ni * h.ld_i);
  h.pitch = ni == 1 ? h.ld_t : h.ld_i;
  return h;
}

// Copy `rows` window time rows starting at window row r0 into dense
// [t][i][span] device memory.
int stage_rows(const HostWin &h, int64_t r0, int64_t rows, void *dstv, hipStream_t st) {
  const int64_t e = h.esz;
  const char *src = h.row0 + r0 * h.ld_t * e;
  char *dst = static_cast<char *>(dstv);
  if (h.uniform) {
    HCHK(hipMemcpy2DAsync(dst, h.span * e, src, h.pitch * e, h.span * e, (size_t)(rows * h.ni),
                          hipMemcpyHostToDevice, st));
  } else {
    for (int64_t r = 0; r < rows; ++r)
      for (int64_t i = 0; i < h.ni; ++i)
        HCHK(hipMemcpyAsync(dst + (r * h.ni + i) * h.span * e, src + (r * h.ld_t + i * h.ld_i) * e,
                            h.span * e, hipMemcpyHostToDevice, st));
  }
  return BLDP_OK;
}

// ---- what the host forms of the block operations share -----------------------
// Each makes its plan call first (every argument check, before any staging),
// takes the counts of the window and of its blocks, refuses its null pointers and
// runs its device entry on the staged window.
// The window's (nc, ni, nt) and its blocks' (nco, ni, nto).
int block_counts(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win, int64_t fqavby,
                 int64_t tavby, int64_t w[3], int64_t o[3]) {
  const int rc = bldp_reduce_shape(nchan, nif, ntime, win, fqavby, tavby, o);
  if (rc) return rc;
  w[0] = o[0] * (fqavby <= 1 ? 1 : fqavby);
  w[1] = o[1];
  w[2] = o[2] * (tavby <= 1 ? 1 : tavby);
  return BLDP_OK;
}

// The strides of a host mask (dense over the window unless given) and its span.
size_t host_mask(const int64_t *mask_ld, const int64_t w[3], int64_t ld[3]) {
  ld[0] = mask_ld ? mask_ld[0] : 1;
  ld[1] = mask_ld ? mask_ld[1] : w[0];
  ld[2] = mask_ld ? mask_ld[2] : w[0] * w[1];
  return bldp::mask_span_bytes(w[0], w[1], w[2], ld);
}

// A device buffer of a staged call: `bytes` in `slot` of the pipeline (0: not
// asked for, p stays null), the first `up_bytes` of it copied from `up`.
struct DevBuf {
  int slot;
  size_t bytes;
  const void *up;
  size_t up_bytes;
  void *p;
};

// The staged copy of a window: its rows dense [t][i][span] at dbuf, i.e. the
// window dwin of a (span, ni, nt) array, on stream st.
struct StagedWin {
  float *dbuf;
  int64_t span;
  int64_t dwin[9];
  bldp::Stager *sg;
  hipStream_t st;
  // a result back into the caller's memory (a null dst was not asked for)
  int fetch(void *dst, const void *src, size_t bytes) const {
    if (dst) HCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return BLDP_OK;
  }
};

// Stage the (nc, ni, nt) window w of `in` and the buffers of `bufs` on `dev`, then
// run body(staged window) on the pipeline's first stream.
template <class Body>
int with_staged_window(int dev, const float *in, int64_t nchan, int64_t nif, const int64_t *win,
                       const int64_t w[3], DevBuf *bufs, int nbufs, Body body) {
  const int64_t nc = w[0], ni = w[1], nt = w[2];
  const HostWin h = host_window(in, 4, nchan, nif, win, nc, ni);
  return with_stager(dev, [&](bldp::Stager *sg) -> int {
    StagedWin s{nullptr, h.span, {h.cs < 0 ? (nc - 1) * h.acs : 0, nc, h.cs, 0, ni, 1, 0, nt, 1},
                sg, sg->st[0]};
    int r = bldp::stager_buffer(sg, 0, (size_t)(h.span * ni * nt) * 4, (void **)&s.dbuf);
    for (int k = 0; k < nbufs && !r; ++k)
      if (bufs[k].bytes) r = bldp::stager_buffer(sg, bufs[k].slot, bufs[k].bytes, &bufs[k].p);
    if (!r) r = stage_rows(h, 0, nt, s.dbuf, s.st);
    if (r) return r;
    for (int k = 0; k < nbufs; ++k)
      if (bufs[k].up_bytes)
        HCHK(hipMemcpyAsync(bufs[k].p, bufs[k].up, bufs[k].up_bytes, hipMemcpyHostToDevice, s.st));
    return body(s);
  });
}

}  // namespace

extern "C" int bldp_reduce_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int64_t fqavby,
                                    int64_t tavby, int op, float *out) {
  int64_t sh[3];
  int rc = bldp_reduce_shape(nchan, nif, ntime, win, fqavby, tavby, sh);
  if (rc) return rc;
  const int64_t nco = sh[0], ni = sh[1], nto = sh[2];
  if (nco * ni * nto == 0) return BLDP_OK;
  if (!in || !out) return bldp::set_error(BLDP_EINVAL, "null pointer");
  const int64_t F = fqavby <= 1 ? 1 : fqavby, T = tavby <= 1 ? 1 : tavby;
  const HostWin h = host_window(in, 4, nchan, nif, win, nco * F, ni);

  // chunk = q output time rows (q*T input rows), ~128 MiB of staged input
  const int64_t row_bytes = h.span * ni * (int64_t)sizeof(float);
  int64_t q = std::max<int64_t>(1, ((int64_t)128 << 20) / std::max<int64_t>(1, row_bytes * T));
  q = std::min(q, nto);
  const int64_t nchunks = (nto + q - 1) / q;
  return with_stager(dev, [&](bldp::Stager *sg) -> int {
    float *dbuf[2], *dout[2];
    for (int b = 0; b < 2 && b < nchunks; ++b) {
      int r = bldp::stager_buffer(sg, b, (size_t)(q * T) * row_bytes, (void **)&dbuf[b]);
      if (!r) r = bldp::stager_buffer(sg, 2 + b, (size_t)(nco * ni * q) * sizeof(float),
                                     (void **)&dout[b]);
      if (r) return r;
    }
    for (int64_t k = 0; k < nchunks; ++k) {
      const int b = (int)(k & 1);
      const int64_t to0 = k * q, qn = std::min(q, nto - to0), rows = qn * T;
      int r = stage_rows(h, to0 * T, rows, dbuf[b], sg->st[b]);
      if (r) return r;
      const int64_t dwin[9] = {h.cs < 0 ? (h.nc - 1) * h.acs : 0, h.nc, h.cs, 0, ni, 1, 0, rows, 1};
      r = bldp_reduce_strided_f32(dbuf[b], h.span, ni, rows, dwin, F, T, op, dout[b], nco,
                                  nco * ni, sg->st[b]);
      if (r) return r;  // message already recorded
      HCHK(hipMemcpyAsync(out + to0 * nco * ni, dout[b], (size_t)(nco * ni * qn) * sizeof(float),
                          hipMemcpyDeviceToHost, sg->st[b]));
    }
    return BLDP_OK;
  });
}

// The host entries of the time-moment family (kurtosis, kurtosis over blocks,
// skewness, moments): stage the window's rows ([t][i][span] dense) on the
// device once with the same copy rules as bldp_reduce_host_f32, run
// `run(dbuf, span, dwin, planes, stream)` there and copy `n` doubles of every
// plane back; a null plane of `out` is neither computed nor copied.
namespace {
template <class Run>
int moments_staged(int dev, const float *in, int64_t nchan, int64_t nif, const int64_t *win,
                   int64_t nc, int64_t ni, int64_t nt, int64_t n, double *const out[4], Run run) {
  const HostWin h = host_window(in, 4, nchan, nif, win, nc, ni);
  int np = 0;
  for (int q = 0; q < 4; ++q) np += out[q] != nullptr;
  return with_stager(dev, [&](bldp::Stager *sg) -> int {
    float *dbuf;
    double *dout;
    int r = bldp::stager_buffer(sg, 0, (size_t)std::max<int64_t>(1, h.span * ni * nt) * 4,
                                (void **)&dbuf);
    if (!r) r = bldp::stager_buffer(sg, 2, (size_t)(np * n) * sizeof(double), (void **)&dout);
    if (!r && nt > 0) r = stage_rows(h, 0, nt, dbuf, sg->st[0]);
    if (r) return r;
    double *d[4];
    for (int q = 0, j = 0; q < 4; ++q) d[q] = out[q] ? dout + (j++) * n : nullptr;
    const int64_t dwin[9] = {h.cs < 0 ? (nc - 1) * h.acs : 0, nc, h.cs, 0, ni, 1, 0, nt, 1};
    r = run(dbuf, h.span, dwin, d, sg->st[0]);
    if (r) return r;  // message already recorded
    for (int q = 0; q < 4; ++q)
      if (out[q])
        HCHK(hipMemcpyAsync(out[q], d[q], (size_t)n * sizeof(double), hipMemcpyDeviceToHost,
                            sg->st[0]));
    return BLDP_OK;
  });
}
}  // namespace

extern "C" int bldp_kurtosis_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                      int64_t ntime, const int64_t *win, double *out) {
  int64_t sh[3];
  int rc = bldp_reduce_shape(nchan, nif, ntime, win, 1, 1, sh);
  if (rc) return rc;
  const int64_t nc = sh[0], ni = sh[1], nt = sh[2];
  if (nc * ni == 0) return BLDP_OK;
  if (!out || (!in && nt > 0)) return bldp::set_error(BLDP_EINVAL, "null pointer");
  double *const o[4] = {out};
  return moments_staged(dev, in, nchan, nif, win, nc, ni, nt, nc * ni, o,
                        [&](const float *d, int64_t span, const int64_t *dwin, double *const *p,
                            hipStream_t s) {
                          return bldp_kurtosis_f32(d, span, ni, nt, dwin, p[0], nullptr, s);
                        });
}

// tblock >= 1: the (nc, ni, nb) kurtosis of every block of tblock spectra.
extern "C" int bldp_kurtosis_blocks_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                             int64_t ntime, const int64_t *win, int64_t tblock,
                                             double *out) {
  int64_t sh[3];
  int rc = bldp_kurtosis_blocks_shape(nchan, nif, ntime, win, tblock, sh);
  if (rc) return rc;
  const int64_t nc = sh[0], ni = sh[1], nb = sh[2], nt = nb * tblock;
  if (nc * ni * nb == 0) return BLDP_OK;
  if (!out || !in) return bldp::set_error(BLDP_EINVAL, "tblock kurtosis: null pointer");
  double *const o[4] = {out};
  return moments_staged(dev, in, nchan, nif, win, nc, ni, nt, nc * ni * nb, o,
                        [&](const float *d, int64_t span, const int64_t *dwin, double *const *p,
                            hipStream_t s) {
                          return bldp_kurtosis_blocks_f32(d, span, ni, nt, dwin, tblock, p[0], nc,
                                                          nc * ni, s);
                        });
}

// tblock = 0 the whole window ((nc, ni) out), tblock >= 1 every block of tblock
// spectra ((nc, ni, nb) out).
extern "C" int bldp_skewness_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                      int64_t ntime, const int64_t *win, int64_t tblock,
                                      double *out) {
  int64_t sh[3], info[4];
  // (every argument check, before any staging)
  int rc = bldp_skewness_plan_f32(nullptr, nchan, nif, ntime, win, tblock, info);
  if (rc) return rc;
  rc = bldp_reduce_shape(nchan, nif, ntime, win, 1, 1, sh);
  if (rc) return rc;
  const int64_t nc = sh[0], ni = sh[1], nt = sh[2], nb = info[2];
  if (nc * ni * nb == 0) return BLDP_OK;
  if (!out || (!in && nt > 0)) return bldp::set_error(BLDP_EINVAL, "skewness: null pointer");
  double *const o[4] = {out};
  return moments_staged(dev, in, nchan, nif, win, nc, ni, nt, nc * ni * nb, o,
                        [&](const float *d, int64_t span, const int64_t *dwin, double *const *p,
                            hipStream_t s) {
                          return bldp_skewness_f32(d, span, ni, nt, dwin, tblock, p[0], nc,
                                                   nc * ni, s);
                        });
}

// Up to four (nc, ni, nb) planes come back.
extern "C" int bldp_moments_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                     int64_t ntime, const int64_t *win, int64_t tblock,
                                     double *mean, double *var, double *skew, double *kurt) {
  int64_t sh[3], info[4];
  // (every argument check, before any staging)
  int rc = bldp_moments_plan_f32(nullptr, nchan, nif, ntime, win, tblock, info);
  if (rc) return rc;
  rc = bldp_reduce_shape(nchan, nif, ntime, win, 1, 1, sh);
  if (rc) return rc;
  const int64_t nc = sh[0], ni = sh[1], nt = sh[2], nb = info[2];
  const int64_t n = nc * ni * nb;
  if (n == 0) return BLDP_OK;
  double *const out[4] = {mean, var, skew, kurt};
  if (!mean && !var && !skew && !kurt)
    return bldp::set_error(BLDP_EINVAL, "moments: every output plane is null");
  if (!in && nt > 0) return bldp::set_error(BLDP_EINVAL, "moments: null pointer");
  for (int q = 0; q < 4; ++q)  // (host planes: the same rule as the device entry's)
    for (int r = q + 1; r < 4; ++r)
      if (out[q] && out[r] && out[q] < out[r] + n && out[r] < out[q] + n)
        return bldp::set_error(BLDP_EINVAL, "moments: output planes overlap");
  return moments_staged(dev, in, nchan, nif, win, nc, ni, nt, n, out,
                        [&](const float *d, int64_t span, const int64_t *dwin, double *const *p,
                            hipStream_t s) {
                          return bldp_moments_f32(d, span, ni, nt, dwin, tblock, p[0], p[1], p[2],
                                                  p[3], nc, nc * ni, s);
                        });
}

// The same staging for tavfunc's var / std / median over blocks of tavby
// spectra: the window's rows go to the device once (in window order: a
// reversed time range is staged reversed), the (nc, ni, nb) product comes back.
extern "C" int bldp_tstat_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                   int64_t ntime, const int64_t *win, int64_t tavby, int op,
                                   float *out) {
  int64_t sh[3];
  int rc = bldp_tstat_shape(nchan, nif, ntime, win, tavby, sh);
  if (rc) return rc;
  // (the op check, before any staging)
  int64_t info[8];
  rc = bldp_tstat_plan_f32(nullptr, nchan, nif, ntime, win, tavby, op, nullptr, info);
  if (rc) return rc;
  const int64_t T = tavby <= 1 ? 1 : tavby;
  const int64_t nc = sh[0], ni = sh[1], nb = sh[2], w[3] = {nc, ni, nb * T};
  if (nc * ni * nb == 0) return BLDP_OK;
  if (!out || !in) return bldp::set_error(BLDP_EINVAL, "tstat: null pointer");
  DevBuf b[1] = {{2, (size_t)(nc * ni * nb) * sizeof(float)}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 1, [&](const StagedWin &s) {
    const int r = bldp_tstat_f32(s.dbuf, s.span, ni, w[2], s.dwin, tavby, op, (float *)b[0].p, nc,
                                 nc * ni, s.st);
    return r ? r : s.fetch(out, b[0].p, b[0].bytes);
  });
}

// Statistics.quantile's index and weight (type 7, alpha = beta = 1) for n >= 2
// values: m = 1 + p (1 - alpha - beta), aleph = n p + m, j = clamp(trunc(aleph),
// 1, n - 1), g = clamp(aleph - j, 0, 1), every operation rounded once (a fused
// n p + m would move g by an ulp); *rank is j - 1.
void bldp::quantile_rank(int64_t n, double p, int64_t *rank, double *g) {
#pragma clang fp contract(off)
  const double m = 1.0 + p * (1.0 - 1.0 - 1.0);
  const double np = (double)n * p;
  const double aleph = np + m;
  const double j = std::min(std::max(std::trunc(aleph), 1.0), (double)(n - 1));
  *rank = (int64_t)j - 1;
  *g = std::min(std::max(aleph - j, 0.0), 1.0);
}

// The same staging for quantile(p) over blocks of n channels (axis 0) or n
// spectra (axis 2): the window's rows go to the device once (in window order),
// the dense product of bldp_quantile_shape comes back.
extern "C" int bldp_quantile_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                      int64_t ntime, const int64_t *win, int axis, int64_t n,
                                      double p, float *out) {
  // (every argument check, before any staging)
  int64_t info[8], sh[3];
  int rc = bldp_quantile_plan_f32(nullptr, nchan, nif, ntime, win, axis, n, p, nullptr, info);
  if (rc) return rc;
  rc = bldp_quantile_shape(nchan, nif, ntime, win, axis, n, sh);
  if (rc) return rc;
  const int64_t nn = n <= 1 ? 1 : n;
  const int64_t nc = axis == 0 ? sh[0] * nn : sh[0], ni = sh[1];
  const int64_t nt = axis == 2 ? sh[2] * nn : sh[2], nout = sh[0] * sh[1] * sh[2];
  if (nout == 0) return BLDP_OK;
  if (!out || !in) return bldp::set_error(BLDP_EINVAL, "quantile: null pointer");
  const int64_t w[3] = {nc, ni, nt};
  DevBuf b[1] = {{2, (size_t)nout * sizeof(float)}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 1, [&](const StagedWin &s) {
    const int r = bldp_quantile_f32(s.dbuf, s.span, ni, nt, s.dwin, axis, n, p, (float *)b[0].p,
                                    sh[0], sh[0] * ni, s.st);
    return r ? r : s.fetch(out, b[0].p, b[0].bytes);
  });
}

// The rank set of quantiles(ps) (bldp_impl.h QSet): quantile_rank per plane,
// then the sorted distinct ranks {j - 1, j}, the sorted distinct lower ranks,
// and where each plane's two ranks lie in them.
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

// The same staging for quantiles(ps): the window's rows go to the device once,
// the np dense planes of bldp_quantiles_shape come back.
extern "C" int bldp_quantiles_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                       int64_t ntime, const int64_t *win, int axis, int64_t n,
                                       int np, const double *p, float *out) {
  // (every argument check, before any staging)
  int64_t info[10], sh[4];
  int rc = bldp_quantiles_plan_f32(nullptr, nchan, nif, ntime, win, axis, n, np, p, nullptr, info);
  if (rc) return rc;
  rc = bldp_quantiles_shape(nchan, nif, ntime, win, axis, n, np, sh);
  if (rc) return rc;
  const int64_t nn = n <= 1 ? 1 : n;
  const int64_t nc = axis == 0 ? sh[0] * nn : sh[0], ni = sh[1];
  const int64_t nt = axis == 2 ? sh[2] * nn : sh[2], plane = sh[0] * sh[1] * sh[2];
  if (plane == 0) return BLDP_OK;
  if (!out || !in) return bldp::set_error(BLDP_EINVAL, "quantiles: null pointer");
  const int64_t w[3] = {nc, ni, nt};
  DevBuf b[1] = {{2, (size_t)(plane * np) * sizeof(float)}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 1, [&](const StagedWin &s) {
    const int r = bldp_quantiles_f32(s.dbuf, s.span, ni, nt, s.dwin, axis, n, np, p,
                                     (float *)b[0].p, sh[0], sh[0] * ni, plane, s.st);
    return r ? r : s.fetch(out, b[0].p, b[0].bytes);
  });
}

// The same staging for outliers: the window's rows go to the device once, the
// dense planes of bldp_outliers_shape that the caller asked for come back.
extern "C" int bldp_outliers_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                      int64_t ntime, const int64_t *win, int axis, int64_t n,
                                      double nsigma, float *med, float *mad, uint32_t *count,
                                      uint8_t *mask) {
  // (every argument check, before any staging)
  int64_t info[10], sh[3], ms[3];
  int rc = bldp_outliers_plan_f32(nullptr, nchan, nif, ntime, win, axis, n, mask != nullptr, info);
  if (rc) return rc;
  if (!(nsigma >= 0.0) || std::isinf(nsigma))
    return bldp::set_error(BLDP_EINVAL, "outliers: nsigma=%g is not a finite number >= 0", nsigma);
  rc = bldp_outliers_shape(nchan, nif, ntime, win, axis, n, sh, ms);
  if (rc) return rc;
  const int64_t nc = ms[0], ni = ms[1], nt = ms[2], plane = sh[0] * sh[1] * sh[2];
  if (plane == 0) return BLDP_OK;
  if (!in) return bldp::set_error(BLDP_EINVAL, "outliers: null input pointer");
  if (!med && !mad && !count && !mask)
    return bldp::set_error(BLDP_EINVAL, "outliers: every output is null");
  // the staged outputs: three planes of 4-byte elements, then the mask
  const size_t pb = (size_t)plane * 4, mb = mask ? (size_t)(nc * ni * nt) : 0;
  DevBuf b[1] = {{2, 3 * pb + mb}};
  return with_staged_window(dev, in, nchan, nif, win, ms, b, 1, [&](const StagedWin &s) {
    char *dout = (char *)b[0].p;
    float *dmed = med ? (float *)dout : nullptr, *dmad = mad ? (float *)(dout + pb) : nullptr;
    uint32_t *dcount = count ? (uint32_t *)(dout + 2 * pb) : nullptr;
    uint8_t *dmask = mask ? (uint8_t *)(dout + 3 * pb) : nullptr;
    int r = bldp_outliers_f32(s.dbuf, s.span, ni, nt, s.dwin, axis, n, nsigma, dmed, dmad, dcount,
                              dmask, sh[0], sh[0] * ni, s.st);
    if (!r) r = s.fetch(med, dmed, pb);
    if (!r) r = s.fetch(mad, dmad, pb);
    if (!r) r = s.fetch(count, dcount, pb);
    if (!r) r = s.fetch(mask, dmask, mb);
    return r;
  });
}

// The same staging for fqavfunc argmax / argmin: the window's rows go to the
// device once (in window order), the (nco, ni, nto) offsets, and the winners'
// bits when val is given, come back.
extern "C" int bldp_argext_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int64_t fqavby,
                                    int64_t tavby, int argop, uint32_t *idx, float *val) {
  // (every argument check, before any staging)
  int64_t info[8];
  int rc = bldp_argext_plan_f32(nullptr, nchan, nif, ntime, win, fqavby, tavby, argop, nullptr,
                                info);
  if (rc) return rc;
  int64_t w[3], o[3];
  rc = block_counts(nchan, nif, ntime, win, fqavby, tavby, w, o);
  if (rc) return rc;
  const size_t nout = (size_t)(o[0] * o[1] * o[2]);
  if (nout == 0) return BLDP_OK;
  if (!in || !idx) return bldp::set_error(BLDP_EINVAL, "argext: null pointer");
  DevBuf b[2] = {{2, nout * sizeof(uint32_t)}, {3, val ? nout * sizeof(float) : 0}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 2, [&](const StagedWin &s) {
    int r = bldp_argext_f32(s.dbuf, s.span, w[1], w[2], s.dwin, fqavby, tavby, argop,
                            (uint32_t *)b[0].p, (float *)b[1].p, o[0], o[0] * o[1], s.st);
    if (!r) r = s.fetch(idx, b[0].p, b[0].bytes);
    if (!r) r = s.fetch(val, b[1].p, b[1].bytes);
    return r;
  });
}

// The same staging for the masked reduce: the window's rows and the mask's span
// (the bytes its strides reach, from the pointer on) go to the device once; the
// dense (nco, ni, nto) outputs that the caller asked for come back.
extern "C" int bldp_masked_reduce_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                           int64_t ntime, const int64_t *win, int64_t fqavby,
                                           int64_t tavby, int op, const uint8_t *mask,
                                           const int64_t *mask_ld, float *out, uint32_t *kept) {
  // (every argument check, before any staging)
  int64_t info[10];
  int rc = bldp_masked_reduce_plan_f32(nullptr, nchan, nif, ntime, win, fqavby, tavby, nullptr,
                                       mask_ld, info);
  if (rc) return rc;
  if (op != BLDP_OP_SUM && op != BLDP_OP_MEAN)
    return bldp::set_error(BLDP_EINVAL, "masked reduce: op %d is not sum (%d) or mean (%d)", op,
                           BLDP_OP_SUM, BLDP_OP_MEAN);
  int64_t w[3], o[3], ld[3];
  rc = block_counts(nchan, nif, ntime, win, fqavby, tavby, w, o);
  if (rc) return rc;
  const size_t nout = (size_t)(o[0] * o[1] * o[2]);
  if (nout == 0) return BLDP_OK;
  if (!in) return bldp::set_error(BLDP_EINVAL, "masked reduce: null input pointer");
  if (!out && !kept)
    return bldp::set_error(BLDP_EINVAL, "masked reduce: out and kept are both null");
  if (!mask) return bldp::set_error(BLDP_EINVAL, "masked reduce: null mask pointer");
  const size_t mb = host_mask(mask_ld, w, ld);
  DevBuf b[3] = {{1, mb, mask, mb}, {2, out ? nout * 4 : 0}, {3, kept ? nout * 4 : 0}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 3, [&](const StagedWin &s) {
    int r = bldp_masked_reduce_f32(s.dbuf, s.span, w[1], w[2], s.dwin, fqavby, tavby, op,
                                   (uint8_t *)b[0].p, ld, (float *)b[1].p, (uint32_t *)b[2].p,
                                   o[0], o[0] * o[1], s.st);
    if (!r) r = s.fetch(out, b[1].p, b[1].bytes);
    if (!r) r = s.fetch(kept, b[2].p, b[2].bytes);
    return r;
  });
}

// The same staging for the histogram: the window's rows go to the device once;
// the dense (nco, ni, nto, nbins + 3) counts come back.
extern "C" int bldp_histogram_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                       int64_t ntime, const int64_t *win, int64_t fqavby,
                                       int64_t tavby, int nbins, double lo, double hi,
                                       uint32_t *out) {
  // (every argument check, before any staging)
  int64_t info[10];
  int rc = bldp_histogram_plan_f32(nullptr, nchan, nif, ntime, win, fqavby, tavby, nbins, lo, hi,
                                   info);
  if (rc) return rc;
  int64_t w[3], o[3];
  rc = block_counts(nchan, nif, ntime, win, fqavby, tavby, w, o);
  if (rc) return rc;
  const int64_t plane = o[0] * o[1] * o[2];
  if (plane == 0) return BLDP_OK;
  if (!in) return bldp::set_error(BLDP_EINVAL, "histogram: null input pointer");
  if (!out) return bldp::set_error(BLDP_EINVAL, "histogram: null output pointer");
  DevBuf b[1] = {{2, (size_t)plane * (size_t)(nbins + 3) * sizeof(uint32_t)}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 1, [&](const StagedWin &s) {
    const int r = bldp_histogram_f32(s.dbuf, s.span, w[1], w[2], s.dwin, fqavby, tavby, nbins, lo,
                                     hi, (uint32_t *)b[0].p, o[0], o[0] * o[1], plane, s.st);
    return r ? r : s.fetch(out, b[0].p, b[0].bytes);
  });
}

// The same staging for the hits list: the window's rows and the mask's span go to
// the device once.  A count-only call gives total; the lists are then sized
// min(total, cap), so the mask is counted twice on the device and the staging
// never holds more than the entries that come back.
extern "C" int bldp_hits_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, const uint8_t *mask,
                                  const int64_t *mask_ld, int64_t cap, int64_t *idx, float *val,
                                  uint64_t *total) {
  // (every argument check, before any staging)
  int64_t info[10];
  int rc = bldp_hits_plan_f32(nullptr, nchan, nif, ntime, win, nullptr, mask_ld, cap, info);
  if (rc) return rc;
  if (!total) return bldp::set_error(BLDP_EINVAL, "hits: null total pointer");
  int64_t w[3], o[3], ld[3];
  rc = block_counts(nchan, nif, ntime, win, 1, 1, w, o);
  if (rc) return rc;
  *total = 0;
  if (w[0] * w[1] * w[2] == 0) return BLDP_OK;
  if (!in) return bldp::set_error(BLDP_EINVAL, "hits: null input pointer");
  if (!mask) return bldp::set_error(BLDP_EINVAL, "hits: null mask pointer");
  const size_t mb = host_mask(mask_ld, w, ld);
  const size_t tot_off = (mb + 7) & ~(size_t)7;  // total sits behind the staged mask
  DevBuf b[1] = {{1, tot_off + sizeof(uint64_t), mask, mb}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 1, [&](const StagedWin &s) -> int {
    uint8_t *dmask = (uint8_t *)b[0].p;
    uint64_t *dtotal = reinterpret_cast<uint64_t *>(dmask + tot_off);
    int r = bldp_hits_f32(s.dbuf, s.span, w[1], w[2], s.dwin, dmask, ld, 0, nullptr, nullptr,
                          dtotal, s.st);
    if (!r) r = s.fetch(total, dtotal, sizeof(uint64_t));
    if (r) return r;
    HCHK(hipStreamSynchronize(s.st));
    const size_t n = (size_t)std::min<uint64_t>(*total, (uint64_t)cap);
    if (n == 0 || (!idx && !val)) return BLDP_OK;
    int64_t *didx = nullptr;
    float *dval = nullptr;
    if (idx) r = bldp::stager_buffer(s.sg, 2, n * sizeof(int64_t), (void **)&didx);
    if (!r && val) r = bldp::stager_buffer(s.sg, 3, n * sizeof(float), (void **)&dval);
    if (!r)
      r = bldp_hits_f32(s.dbuf, s.span, w[1], w[2], s.dwin, dmask, ld, (int64_t)n, didx, dval,
                        dtotal, s.st);
    if (!r) r = s.fetch(idx, didx, n * sizeof(int64_t));
    if (!r) r = s.fetch(val, dval, n * sizeof(float));
    return r;
  });
}

// The same staging for the fold: the window's rows and (where there is one) the
// mask's span go to the device once; the dense (nfpc, ni, nto) outputs that the
// caller asked for come back.
extern "C" int bldp_fold_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby,
                                  int op, const uint8_t *mask, const int64_t *mask_ld, float *out,
                                  uint32_t *kept) {
  // (every argument check, before any staging)
  int64_t info[10];
  int rc = bldp_fold_plan_f32(nullptr, nchan, nif, ntime, win, nfpc, tavby, nullptr,
                              mask ? mask_ld : nullptr, info);
  if (rc) return rc;
  if (op != BLDP_OP_SUM && op != BLDP_OP_MEAN)
    return bldp::set_error(BLDP_EINVAL, "fold: op %d is not sum (%d) or mean (%d)", op,
                           BLDP_OP_SUM, BLDP_OP_MEAN);
  int64_t sh[3], w[3], o[3], ld[3];
  rc = bldp_fold_shape(nchan, nif, ntime, win, nfpc, tavby, sh);
  if (!rc) rc = block_counts(nchan, nif, ntime, win, 1, 1, w, o);
  if (rc) return rc;
  const int64_t ni = w[1];
  const size_t nout = (size_t)(sh[0] * ni * sh[2]);
  if (nout == 0) return BLDP_OK;
  if (!in) return bldp::set_error(BLDP_EINVAL, "fold: null input pointer");
  if (!out && !kept) return bldp::set_error(BLDP_EINVAL, "fold: out and kept are both null");
  const size_t span = host_mask(mask_ld, w, ld), mb = mask ? span : 0;
  DevBuf b[3] = {{1, mb, mask, mb}, {2, out ? nout * 4 : 0}, {3, kept ? nout * 4 : 0}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 3, [&](const StagedWin &s) {
    int r = bldp_fold_f32(s.dbuf, s.span, ni, w[2], s.dwin, nfpc, tavby, op, (uint8_t *)b[0].p, ld,
                          (float *)b[1].p, (uint32_t *)b[2].p, nfpc, nfpc * ni, s.st);
    if (!r) r = s.fetch(out, b[1].p, b[1].bytes);
    if (!r) r = s.fetch(kept, b[2].p, b[2].bytes);
    return r;
  });
}

// ... and for the unfold: the window's rows and the dense (nfpc, ni, nto) profile
// go to the device once; the dense (nc, ni, nt) result comes back.
extern "C" int bldp_unfold_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int64_t nfpc,
                                    int64_t tavby, int uop, const float *prof, float *out) {
  // (every argument check, before any staging)
  int64_t sh[3], w[3], o[3];
  int rc = bldp_fold_shape(nchan, nif, ntime, win, nfpc, tavby, sh);
  if (!rc) rc = block_counts(nchan, nif, ntime, win, 1, 1, w, o);
  if (rc) return rc;
  if (uop != BLDP_UNFOLD_DIV && uop != BLDP_UNFOLD_SUB)
    return bldp::set_error(BLDP_EINVAL, "unfold: op %d is not divide (%d) or subtract (%d)", uop,
                           BLDP_UNFOLD_DIV, BLDP_UNFOLD_SUB);
  const int64_t nc = w[0], ni = w[1], nt = w[2];
  if (nc * ni * nt == 0) return BLDP_OK;
  if (!in) return bldp::set_error(BLDP_EINVAL, "unfold: null input pointer");
  if (!prof) return bldp::set_error(BLDP_EINVAL, "unfold: null profile pointer");
  if (!out) return bldp::set_error(BLDP_EINVAL, "unfold: null output pointer");
  const size_t pbytes = (size_t)(nfpc * ni * sh[2]) * 4;
  DevBuf b[2] = {{1, pbytes, prof, pbytes}, {2, (size_t)(nc * ni * nt) * 4}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 2, [&](const StagedWin &s) {
    const int r = bldp_unfold_f32(s.dbuf, s.span, ni, nt, s.dwin, nfpc, tavby, uop,
                                  (float *)b[0].p, nfpc, nfpc * ni, (float *)b[1].p, nc, nc * ni,
                                  s.st);
    return r ? r : s.fetch(out, b[1].p, b[1].bytes);
  });
}

// ... and for the dedoppler: the window's rows go to the device once; the dense
// (nc, ni, nb) best and drift and the dense (nc, ni, nb, 2*maxdrift + 1) sums that
// the caller asked for come back.
extern "C" int bldp_dedoppler_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                       int64_t ntime, const int64_t *win, int64_t tavby,
                                       int64_t maxdrift, int64_t seg, float *best, int *drift,
                                       float *sums) {
  // (every argument check, before any staging)
  int64_t info[10];
  int rc = bldp_dedoppler_plan_f32(nullptr, nchan, nif, ntime, win, tavby, maxdrift, seg, info);
  if (rc) return rc;
  int64_t w[3], o[3];
  rc = block_counts(nchan, nif, ntime, win, 1, tavby, w, o);
  if (rc) return rc;
  const size_t plane = (size_t)(o[0] * o[1] * o[2]);
  if (plane == 0) return BLDP_OK;
  if (!in) return bldp::set_error(BLDP_EINVAL, "dedoppler: null input pointer");
  if ((best == nullptr) != (drift == nullptr))
    return bldp::set_error(BLDP_EINVAL, "dedoppler: best and drift go together");
  if (!best && !sums)
    return bldp::set_error(BLDP_EINVAL, "dedoppler: best / drift and sums are all null");
  const size_t K = (size_t)(2 * maxdrift + 1);
  DevBuf b[3] = {{2, best ? plane * 4 : 0}, {3, drift ? plane * 4 : 0}, {1, sums ? plane * K * 4 : 0}};
  return with_staged_window(dev, in, nchan, nif, win, w, b, 3, [&](const StagedWin &s) {
    int r = bldp_dedoppler_f32(s.dbuf, s.span, w[1], w[2], s.dwin, tavby, maxdrift, seg,
                               (float *)b[0].p, (int *)b[1].p, (float *)b[2].p, o[0],
                               o[0] * o[1], (int64_t)plane, s.st);
    if (!r) r = s.fetch(best, b[0].p, b[0].bytes);
    if (!r) r = s.fetch(drift, b[1].p, b[1].bytes);
    if (!r) r = s.fetch(sums, b[2].p, b[2].bytes);
    return r;
  });
}

// ---------------------------------------------------------------------------
// Host forms of the typed entry points (include/bldp.h), staged like the
// Float32 forms above: only the window's rows (its channel span of every
// selected (IF, spectrum) row) cross to the device, dense [t][i][span], so a
// narrow window of a large mmap'ed SIGPROC file moves the window, not the file.
// The reduce runs in chunks of whole output time rows on the two streams of a
// pooled staging pipeline; the kurtosis, which needs every spectrum of a row,
// stages the window once.  Synchronous.
extern "C" int bldp_reduce_host(int dev, int dtype, const void *in, int64_t nchan, int64_t nif,
                                int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                                int op, void *out) {
  if (dtype == BLDP_DT_F32)
    return bldp_reduce_host_f32(dev, static_cast<const float *>(in), nchan, nif, ntime, win,
                                fqavby, tavby, op, static_cast<float *>(out));
  const int od = bldp_reduce_out_dtype(dtype, op);
  if (od < 0) return od;
  if (bldp::stat_op(op))  // (before anything is staged)
    return bldp::set_error(BLDP_EINVAL,
                           "median/var/std/mad take Float32 on the GPU (element type %d)", dtype);
  int64_t sh[3];
  int rc = bldp_reduce_shape(nchan, nif, ntime, win, fqavby, tavby, sh);
  if (rc) return rc;
  const int64_t nco = sh[0], ni = sh[1], nto = sh[2];
  if (nco * ni * nto == 0) return BLDP_OK;
  if (!in || !out) return bldp::set_error(BLDP_EINVAL, "null pointer");
  const int64_t esz = (int64_t)bldp::dtype_size(dtype), osz = (int64_t)bldp::dtype_size(od);
  const int64_t F = fqavby <= 1 ? 1 : fqavby, T = tavby <= 1 ? 1 : tavby;
  const HostWin h = host_window(in, esz, nchan, nif, win, nco * F, ni);
  const int64_t row_bytes = h.span * ni * esz;
  int64_t q = std::max<int64_t>(1, ((int64_t)128 << 20) / std::max<int64_t>(1, row_bytes * T));
  q = std::min(q, nto);
  const int64_t nchunks = (nto + q - 1) / q;
  return with_stager(dev, [&](bldp::Stager *sg) -> int {
    void *dbuf[2], *dout[2];
    for (int b = 0; b < 2 && b < nchunks; ++b) {
      int r = bldp::stager_buffer(sg, b, (size_t)(q * T * row_bytes), &dbuf[b]);
      if (!r) r = bldp::stager_buffer(sg, 2 + b, (size_t)(nco * ni * q * osz), &dout[b]);
      if (r) return r;
    }
    for (int64_t k = 0; k < nchunks; ++k) {
      const int b = (int)(k & 1);
      const int64_t to0 = k * q, qn = std::min(q, nto - to0), rows = qn * T;
      int r = stage_rows(h, to0 * T, rows, dbuf[b], sg->st[b]);
      if (r) return r;
      const int64_t dwin[9] = {h.cs < 0 ? (h.nc - 1) * h.acs : 0, h.nc, h.cs, 0, ni, 1, 0, rows, 1};
      r = bldp_reduce_strided(dtype, dbuf[b], h.span, ni, rows, dwin, F, T, op, dout[b], nco,
                              nco * ni, sg->st[b]);
      if (r) return r;
      HCHK(hipMemcpyAsync(static_cast<char *>(out) + to0 * nco * ni * osz, dout[b],
                          (size_t)(nco * ni * qn * osz), hipMemcpyDeviceToHost, sg->st[b]));
    }
    return BLDP_OK;
  });
}

extern "C" int bldp_kurtosis_host(int dev, int dtype, const void *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, double *out) {
  if (dtype == BLDP_DT_F32)
    return bldp_kurtosis_host_f32(dev, static_cast<const float *>(in), nchan, nif, ntime, win,
                                  out);
  if (!bldp::dtype_size(dtype)) return bldp::set_error(BLDP_EINVAL, "unknown element type %d", dtype);
  int64_t sh[3];
  int rc = bldp_reduce_shape(nchan, nif, ntime, win, 1, 1, sh);
  if (rc) return rc;
  const int64_t nc = sh[0], ni = sh[1], nt = sh[2];
  if (nc * ni == 0) return BLDP_OK;
  if (!out) return bldp::set_error(BLDP_EINVAL, "null pointer");
  if (nt == 0) {  // no spectra: every row NaN (mean of nothing), as the Float32 path
    for (int64_t k = 0; k < nc * ni; ++k) out[k] = NAN;
    return BLDP_OK;
  }
  if (!in) return bldp::set_error(BLDP_EINVAL, "null pointer");
  const int64_t esz = (int64_t)bldp::dtype_size(dtype);
  const HostWin h = host_window(in, esz, nchan, nif, win, nc, ni);
  return with_stager(dev, [&](bldp::Stager *sg) -> int {
    void *dbuf, *dout;
    int r = bldp::stager_buffer(sg, 0, (size_t)(h.span * ni * nt * esz), &dbuf);
    if (!r) r = bldp::stager_buffer(sg, 2, (size_t)(nc * ni) * sizeof(double), &dout);
    if (!r) r = stage_rows(h, 0, nt, dbuf, sg->st[0]);
    if (r) return r;
    const int64_t dwin[9] = {h.cs < 0 ? (nc - 1) * h.acs : 0, nc, h.cs, 0, ni, 1, 0, nt, 1};
    r = bldp_kurtosis(dtype, dbuf, h.span, ni, nt, dwin, static_cast<double *>(dout), sg->st[0]);
    if (r) return r;
    HCHK(hipMemcpyAsync(out, dout, (size_t)(nc * ni) * sizeof(double), hipMemcpyDeviceToHost,
                        sg->st[0]));
    return BLDP_OK;
  });
}
