/*
 * bldp.h — C ABI of libbldp_hip, the MI355X engine for the worker-side
 * reduction of BLDistributedDataProducts.jl (reference v0.3.2).
 *
 * Every entry point here replaces one piece of the reference's Julia hot path
 * (paths are relative to the reference repo root):
 *
 *   bldp_reduce_f32        fqav(A, n; f) src/gbtworkerfunctions.jl:16-20, applied
 *                          to the window read at :182-186 / :173-174, plus the
 *                          additive time integration (fqav on axis 3).
 *   bldp_reduce_host_f32   same, for a host array (what WorkerFunctions.getdata
 *                          holds after the HDF5/mmap read, :174 / :188).
 *   bldp_band_reduce_f32   GBT.getdata fan-out (src/gbt.jl:69-79) + the band
 *                          stitch reduce(vcat, ...) (src/gbt.jl:103) for banks
 *                          resident on one GPU.
 *   bldp_stitch_f32        reduce(vcat, banks) (src/gbt.jl:103) of bank-major
 *                          gathered blocks.
 *   bldp_comm_* /          GBT.getdata's fetch of every worker's result to the
 *   bldp_band_gather_f32   caller (src/gbt.jl:75-78) as an RCCL gather over xGMI.
 *   bldp_despike_f32       d[spike:nfpc:end,:,:] .= d[spike-1:nfpc:end,:,:]
 *                          (src/gbt.jl:101-102,111).
 *   bldp_kurtosis_f32      getkurtosis (src/gbtworkerfunctions.jl:197-202) with
 *                          StatsBase.kurtosis' two-pass recipe.
 *   bldp_fqav_range        fqav(r::AbstractRange, n) src/gbtworkerfunctions.jl:27-33.
 *   bldp_bslz4_*           HDF5 filter 32008 decode behind h5["data"][idxs...]
 *                          (:181-187; H5Zbitshuffle, Project.toml:10).
 *
 * Conventions
 *   - Arrays are Julia column-major (nchan, nif, ntime), channel fastest
 *     (README.md:165-168); in C terms data[t][i][c].
 *   - A window is 9 int64: {c0, nc, cs, i0, ni, is, t0, nt, ts} = 0-based
 *     start, count and step per axis (a Julia range a:s:b becomes start=a-1,
 *     count=length, step=s).  NULL means the whole array, i.e. idxs=(:,:,:).
 *   - fqavby <= 1 / tavby <= 1 disable that axis (fqav returns A, :17).
 *     fqavby must divide nc (Julia reshape -> DimensionMismatch, :18-19);
 *     tavby must divide nt (same rule on axis 3).  Both give BLDP_EDIM.
 *   - "_f32" device entry points take DEVICE pointers and a hipStream_t passed
 *     as void* (NULL = the null stream).  They are asynchronous on that stream
 *     and never synchronize; buffers are owned by the caller.
 *   - Return value 0 = ok, negative = error; bldp_last_error() returns the
 *     thread-local message of the last failing call.
 *
 * Threading ("reentrant per device handle")
 *   - Every entry point may be called from several host threads at once, for
 *     the same or different devices (GBT.getdata's per-worker fan-out,
 *     src/gbt.jl:75-77).  Library state shared between calls (per-(device,
 *     stream) scratch, staging pipelines, pinned slot rings, reader threads)
 *     is leased per call under its own lock; results never depend on what
 *     another thread is doing.
 *   - The only process-wide mutable setting is bldp_plan_option, an A/B and
 *     test facility: the product path never sets it, and a caller that sets
 *     it changes the kernel choice (never the results: every form is
 *     bit-identical or held to the same tolerance) of every thread's later
 *     plans.  Choices that are part of a call (e.g. the staged branch of
 *     bldp_band_reduce_multi_f32) are arguments of that call.
 *   - Asynchronous entry points order their work on the caller's stream only;
 *     a caller that hands data between streams or threads does the ordering
 *     (events) itself.
 */
#ifndef BLDP_H
#define BLDP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: bldp_bslz4_decode_dev / _async take out_len (round 2); BLDP_EIO; the
 *    typed (non-Float32) entry points
 * 3: prepared band reduces (bldp_band_reduce_prepare_f32 / bldp_reduce_launch /
 *    bldp_reduce_launch_timed / bldp_reduce_release); bldp_plan_option; bldp_file_runs_to_device
 * 4: bldp_band_reduce_multi_f32 takes a flags word (BLDP_BAND_STAGED replaces
 *    the process-wide "force_staged" option and BLDP_FORCE_STAGED);
 *    bldp_peer_access; bldp_device_to_host; bldp_file_chunks_to_device;
 *    bldp_chunks_to_device stages through the pinned slot ring when
 *    host_pinned is NULL;
 *    bldp_plan_option checks each
 *    option's domain; bldp_read_probe moved out of the product library
 *    (tools/hbm_probe.hip, build/libbldp_probe.so); plan options
 *    "force_staged", "il_persist", "max_wg_per_cu", "typed_rows" removed, and
 *    the values that only ever forced a losing form (narrow_mis 2, lane 2,
 *    wavet 2, unaligned_vec 3, kurt_leaf_tile 2)
 * 5: bldp_reduce_prepare / bldp_kurtosis_prepare (any element type) launched
 *    by bldp_reduce_launch; bldp_band_reduce_multi_f32 flag
 *    BLDP_BAND_PEER_STORE (direct xGMI stores are opt-in); plan option
 *    "typed_kurt"; (additive, same version) bldp_op gains BLDP_OP_VAR,
 *    BLDP_OP_STD, BLDP_OP_MEDIAN for the Float32 reduce entry points; the
 *    bldp_kurtosis_blocks_*, bldp_tstat_*, bldp_argext_*, bldp_skewness_* and
 *    bldp_moments_* entry points; (additive, same version) BLDP_OP_MAD = 8
 *    wherever BLDP_OP_MEDIAN is taken (7 stays unassigned and invalid);
 *    (additive, same version) the bldp_quantile_* entry points;
 *    (additive, same version) the bldp_quantiles_* entry points;
 *    (additive, same version) the bldp_outliers_* entry points;
 *    (additive, same version) the bldp_*masked_reduce_* entry points;
 *    (additive, same version) the bldp_*histogram_* entry points;
 *    (additive, same version) the bldp_*hits_* entry points;
 *    (additive, same version) the bldp_*fold_* and bldp_*unfold_* entry points;
 *    (additive, same version) the bldp_*dedoppler_* entry points */
#define BLDP_ABI_VERSION 5

#if defined(BLDP_BUILD)
#define BLDP_API __attribute__((visibility("default")))
#else
#define BLDP_API
#endif

/* fqavfunc values named by README.md:192-195, and its "etc.": Statistics'
 * var (corrected), std and median over the fqavby channels of a block.  Those
 * three take Float32 data and no time integration (tavby <= 1, else
 * BLDP_EINVAL); Float32 in, Float32 out.  median orders by isless
 * (-0.0 < 0.0), returns the middle element of an odd block and
 * middle(a, b) = a/2 + b/2 of an even one, and NaN for a block holding a NaN.
 * BLDP_OP_MAD is the normalised median absolute deviation (StatsBase's
 * mad(x; normalize=true)) under the same conditions: c = median(x), then the
 * median (same rule, NaN wins again) of d = |x - c| with the difference
 * rounded once to Float32, times 1.4826022185056018 in Float64 and rounded to
 * Float32.  fqavby <= 1 copies the window, as for every op.  7 is unassigned
 * and BLDP_EINVAL everywhere. */
enum bldp_op {
  BLDP_OP_SUM = 0, BLDP_OP_MEAN = 1, BLDP_OP_MAX = 2, BLDP_OP_MIN = 3,
  BLDP_OP_VAR = 4, BLDP_OP_STD = 5, BLDP_OP_MEDIAN = 6,
  BLDP_OP_MAD = 8
};

/* error codes */
#define BLDP_OK 0
#define BLDP_EINVAL (-1)  /* bad argument / AssertionError analogue            */
#define BLDP_EDIM (-2)    /* DimensionMismatch: fqavby/tavby does not divide     */
#define BLDP_EHIP (-3)    /* HIP runtime error                                   */
#define BLDP_ENOMEM (-5)  /* device or pinned allocation failed                  */
#define BLDP_EBOUNDS (-6) /* window outside the array (BoundsError analogue)     */
#define BLDP_ECOMM (-7)   /* RCCL error in the cross-GPU band exchange          */
#define BLDP_EIO (-8)     /* a file read failed or ended early (truncated file)  */

#define BLDP_MAX_BANKS 64

BLDP_API int bldp_abi_version(void);
/* Copy the last error message of this thread into buf (NUL-terminated). */
BLDP_API int bldp_last_error(char *buf, size_t len);
/* Number of visible GPUs. */
BLDP_API int bldp_device_count(int *n);

/* Library setup (SURVEY §8 B2 bldp_init/bldp_finalize; called where the
 * reference sets up its workers, GBT.setupworkers, src/gbt.jl:12-46).
 * devs == NULL selects every visible device.  Checks each device is gfx950
 * (BLDP_EINVAL otherwise), creates its worker stream and one warm
 * host-staging pipeline, and enables peer access between the listed devices.
 * Optional: every entry point initialises what it needs on first use. */
BLDP_API int bldp_init(int ndev, const int *devs);
/* Drain the devices and free every library-owned resource (scratch,
 * staging pipelines, streams).  BLDP_EINVAL while a host call is running.
 * Later calls re-initialise lazily. */
BLDP_API int bldp_finalize(void);
/* Page-lock / unlock a long-lived caller host buffer so the host-array entry
 * points copy from it at full PCIe rate (hipHostRegister). */
BLDP_API int bldp_host_register(void *ptr, size_t bytes);
BLDP_API int bldp_host_unregister(void *ptr);

/* Output shape of a reduction: nco = nc/F, nto = nt/T (after the divisibility
 * checks), ni = window IF count.  Pure host function. */
BLDP_API int bldp_reduce_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                      int64_t fqavby, int64_t tavby, int64_t out_shape[3]);

/* Introspection (tests/bench): the launch plan bldp_reduce_f32 would use for
 * these pointers.  info = {path (0 vector, 1 narrow, 2 scalar, 3 tile,
 * 4 interleaved, 5 row, 6 narrow_mis, 7 lane; var / std: 8 moments; median:
 * 9 bitonic sort of blocks <= 64, 10 radix select with the keys in registers,
 * 11 radix select re-reading the block; mad: the median's path for its shape,
 * the selection run twice), lanes per group (8-11: 256 = one
 * workgroup per block), waves (row
 * path: workgroup slices) splitting T, float4 per lane per row, time chunks,
 * workgroups, workspace bytes, vector output stores}.  Launches nothing. */
BLDP_API int bldp_reduce_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                         const int64_t *win, int64_t fqavby, int64_t tavby, int op,
                         const float *out, int64_t info[8]);

/* Process-wide plan options, an A/B and TEST facility only (see Threading
 * above: the product path never sets one): override one of the planners'
 * measured choices.  value -1 restores the default; *previous (may be NULL)
 * receives the old override (-1 = none).  Every form is parity-tested
 * (tests/test_gpu_parity.py::test_plan_options_every_form).
 *   "row_split"      k_reduce_row's time block over 1, 2 or 4 slices of a
 *                    workgroup (whole 16-row batches only; bit-identical
 *                    forms); default -1 = chosen by launch size
 *   "ts_fill", "narrow_mis", "t38", "wide_split",
 *   "narrow_tpb", "lane", "lane3", "lanet", "lanet_pack", "vec_il",
 *   "vec_row", "row_tpb", "rowt_pack", "rowt_small", "wavet",
 *   "unaligned_vec", "kurt_exact", "kurt_mid_cpl", "kurt_mid_small",
 *   "kurt_leaf_narrow", "kurt_leaf_tile", "typed_vec", "typed_kurt",
 *   "row_bpack", "lane_bpack", "wave_bpack", "col3", "rowt_narrow8", "st_plain"
 *                    which kernel a reduce / kurtosis / typed shape takes
 *                    (csrc/kernels.hip kPlanOpts: defaults, meanings and the
 *                    values each option accepts).
 * Unknown names, and values outside an option's domain: BLDP_EINVAL. */
BLDP_API int bldp_plan_option(const char *name, int64_t value, int64_t *previous);

/* out[c', i, t'] = op over the F x T block of the window (device pointers).
 * out is dense (nco, ni, nto). */
BLDP_API int bldp_reduce_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                    const int64_t *win, int64_t fqavby, int64_t tavby, int op, float *out,
                    void *stream);

/* Same with an explicit output layout: element (c', i, t') is written at
 * out[c' + out_ld_i * i + out_ld_t * t'] (lets a bank write straight into
 * its slot of a stitched band product). */
BLDP_API int bldp_reduce_strided_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                            const int64_t *win, int64_t fqavby, int64_t tavby, int op,
                            float *out, int64_t out_ld_i, int64_t out_ld_t, void *stream);

/* Host-pointer form: in and out are host memory; the window is streamed to
 * device `dev` through double-buffered staging and reduced there.
 * Synchronous (returns when out is filled). */
BLDP_API int bldp_reduce_host_f32(int dev, const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                         const int64_t *win, int64_t fqavby, int64_t tavby, int op, float *out);

/* Band of nbank banks on ONE device, all with the same (nchan, nif, ntime)
 * and window: reduces every bank and writes the stitched product
 * out (nbank*nco, ni, nto) in bank order, i.e. reduce(vcat, ...) of the
 * per-bank results (src/gbt.jl:103).  in[] is a HOST array of device
 * pointers.  One launch covers every bank. */
BLDP_API int bldp_band_reduce_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                         int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                         int op, float *out, void *stream);

/* bldp_band_reduce_f32 prepared once for fixed buffers: the argument checks,
 * window, launch plan and kernel arguments are computed here, so each
 * bldp_reduce_launch only queues the kernel(s) on `stream` (same results as
 * bldp_band_reduce_f32 with these arguments).  The handle is bound to the
 * current device and to these pointers; the caller keeps them alive until
 * bldp_reduce_release.  Same errors as bldp_band_reduce_f32 at prepare time;
 * a launch from another current device is BLDP_EINVAL. */
typedef struct bldp_reduce_op *bldp_reduce_op_t;
BLDP_API int bldp_band_reduce_prepare_f32(int nbank, const float *const *in, int64_t nchan,
                                          int64_t nif, int64_t ntime, const int64_t *win,
                                          int64_t fqavby, int64_t tavby, int op, float *out,
                                          bldp_reduce_op_t *handle);
BLDP_API int bldp_reduce_launch(bldp_reduce_op_t handle, void *stream);
/* bldp_reduce_launch with timing: the reduce's own kernel dispatches carry
 * the events (hipExtLaunchKernel), `ev_start` taking the first dispatch's
 * start and `ev_stop` the last one's end, so timing a launch queues nothing
 * between it and the next.  Both are hipEvent_t created with timing enabled;
 * read them with hipEventElapsedTime.  An empty reduce records neither. */
BLDP_API int bldp_reduce_launch_timed(bldp_reduce_op_t handle, void *stream, void *ev_start,
                                      void *ev_stop);
BLDP_API int bldp_reduce_release(bldp_reduce_op_t handle);

/* One process, one or more banks per GPU: bank b lives on
 * device bank_dev[b] (in[b] is a device pointer there).  Every device reduces
 * its banks into their vcat slots of `out`, the stitched (nbank*nco, ni, nto)
 * product on device `root`.  A device's banks are reduced by one launch per
 * run of evenly spaced bank indices (one launch per device for contiguous
 * shards).  The root's kernels store their slots directly; another device's
 * banks are reduced into library staging on that device and moved by one
 * strided peer copy per run (DMA over xGMI).  Synchronous; all banks share the
 * same (nchan, nif, ntime) and window.  Replaces the per-worker getdata +
 * reduce(vcat, ...) of GBT.getdata / loadscan (src/gbt.jl:75-78,103).
 * flags: 0, or one of
 *   BLDP_BAND_STAGED      every bank takes the staged branch, the root's banks
 *                         included (how a one-GPU box runs that branch);
 *   BLDP_BAND_PEER_STORE  devices with peer access to `root` store their
 *                         slots directly from the reduce kernels (xGMI
 *                         stores, no staging copy).  Opt-in: this branch has
 *                         not yet run on a multi-GPU node. */
#define BLDP_BAND_STAGED 1u
#define BLDP_BAND_PEER_STORE 2u
BLDP_API int bldp_band_reduce_multi_f32(int nbank, const int *bank_dev, const float *const *in,
                                        int64_t nchan, int64_t nif, int64_t ntime,
                                        const int64_t *win, int64_t fqavby, int64_t tavby,
                                        int op, int root, float *out, unsigned flags);

/* Whether kernels running on device `dev` may store straight into memory of
 * device `peer` (the same device, or peer access over xGMI, which this call
 * enables when the hardware allows it): *direct = 1, else 0 (the caller stages
 * and copies).  What GBT.getband's bank-by-bank branch asks before a bank's
 * reduce on its own GPU writes the root's vcat slot (src/gbt.jl:103). */
BLDP_API int bldp_peer_access(int dev, int peer, int *direct);

/* Device -> host copy of `bytes` from src (memory of the current device) into
 * ordinary (pageable) host memory dst through the library's ring of pinned
 * slots (the current device's, shared with the file readers): slot-sized DMA
 * copies on copy_stream, each landed slot copied out to dst by the reader
 * threads while the next DMA runs.  The copies start after the work queued so
 * far on `stream` (the producer's stream).  Synchronous: returns when dst is
 * filled.  No pinned memory is allocated per call, and dst is never
 * page-locked.  stats (NULL or 4 doubles): ms to the first DMA, total ms,
 * slots, copy-out threads. */
BLDP_API int bldp_device_to_host(const void *src, void *dst, int64_t bytes, void *copy_stream,
                                 void *stream, double *stats);

/* Band stitch across processes, one GPU each (the reference's one
 * Distributed.jl worker per bank, src/gbt.jl:75-77): an RCCL communicator
 * and ncclGather over xGMI (RCCL is loaded at run time).
 *   rank 0: bldp_comm_id(id), sends the 128 bytes to every rank;
 *   every rank: bldp_comm_init (collective), reduces its banks into a dense
 *   slice with bldp_band_reduce_f32, then bldp_band_gather_f32: the root's
 *   `gathered` receives nranks slices of `count` floats, rank-major;
 *   root: bldp_stitch_f32(nranks, gathered, ...) puts rank-major slices in
 *   vcat order (no-op layout when every bank's output is one (IF, time) row).
 * The gather is asynchronous on `stream`. */
#define BLDP_COMM_ID_BYTES 128
BLDP_API int bldp_comm_id(uint8_t id[BLDP_COMM_ID_BYTES]);
BLDP_API int bldp_comm_init(int dev, int nranks, int rank, const uint8_t id[BLDP_COMM_ID_BYTES],
                            void **comm);
BLDP_API int bldp_comm_destroy(void *comm);
BLDP_API int bldp_band_gather_f32(void *comm, int root, const float *slice, int64_t count,
                                  float *gathered, void *stream);

/* gathered: nbank dense blocks (nc, nif, ntime) back to back (bank-major,
 * what a gather to the root leaves); out: (nbank*nc, nif, ntime) = vcat. */
BLDP_API int bldp_stitch_f32(int nbank, const float *gathered, int64_t nc, int64_t nif, int64_t ntime,
                    float *out, void *stream);

/* In place on data (nchan, nif, ntime): for every coarse channel the DC bin
 * (0-based nfpc/2) takes the value of its left neighbour. nfpc >= 2. */
BLDP_API int bldp_despike_f32(float *data, int64_t nchan, int64_t nif, int64_t ntime, int64_t nfpc,
                     void *stream);

/* Excess kurtosis over time of every (channel, if) row of the window.
 * out is (nc, ni) float64 on the device. workspace: device scratch of
 * bldp_kurtosis_workspace_size() bytes, or NULL for a library-cached one. */
BLDP_API size_t bldp_kurtosis_workspace_size(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win);
/* Introspection (tests/bench): the kurtosis plan for this pointer and window.
 * info = {path (0 registers, 1 register tile, 2 streamed leaves + tree
 * merge, 3 two passes), K (level of the pairwise-sum blocks), leaf slots,
 * workspace bytes}.  Launches nothing. */
BLDP_API int bldp_kurtosis_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                    const int64_t *win, int64_t info[4]);
BLDP_API int bldp_kurtosis_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                      const int64_t *win, double *out, void *workspace, void *stream);

/* Kurtosis of every bank of a band resident on one device, one set of
 * launches for all banks (the GBT.getkurtosis fan-out, src/gbt.jl:81-88).
 * in[] is a HOST array of device pointers; out is nbank (nc, ni) float64
 * matrices back to back on the device. */
BLDP_API int bldp_band_kurtosis_f32(int nbank, const float *const *in, int64_t nchan,
                                    int64_t nif, int64_t ntime, const int64_t *win, double *out,
                                    void *stream);

/* Host-pointer form of bldp_kurtosis_f32 for a worker holding the data in
 * host memory: the window is staged on device `dev`, out (nc, ni) float64 is
 * host memory.  Synchronous. */
BLDP_API int bldp_kurtosis_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, double *out);

/* Kurtosis over blocks of spectra (getkurtosis(...; tblock)): the window's
 * selected spectra are cut into nb = nt / tblock blocks, block b holding
 * spectra [b*tblock, (b+1)*tblock), and element (c, i, b) of the (nc, ni, nb)
 * float64 result is what bldp_kurtosis_f32 gives for block b alone (the same
 * recipe, Base.sum's Float32 mean of the block).  tblock < 1 is BLDP_EINVAL,
 * a tblock that does not divide nt BLDP_EDIM (the rule of tavby).  Additive in
 * ABI 5.
 *
 * Float4-column windows (unit channel step, channel count a multiple of 4)
 * with tblock <= 1024 run in one launch with no workspace: tblock <= 32
 * bit-identical to the recipe, longer blocks with the moments exact in
 * Float64 (the "leaf" class).  Every other shape runs block by block through
 * the paths of bldp_kurtosis_f32 inside the call, on `stream`, with library
 * scratch leased once.  Asynchronous.
 *
 * bldp_kurtosis_blocks_shape: dims = {nc, ni, nb}; every argument check.
 * bldp_kurtosis_blocks_plan_f32: info = {path of the blocks (as
 * bldp_kurtosis_plan_f32), 1 = the one-launch form / 0 = block by block, nb,
 * workspace bytes}; launches nothing and needs no GPU.
 * bldp_kurtosis_blocks_f32: element (c, i, b) at out[c + i*out_ld_i +
 * b*out_ld_b] (elements; dense = (nc, nc*ni)).
 * bldp_band_kurtosis_blocks_f32: in[] is a HOST array of device pointers; out
 * is dense [nbank][nb][ni][nc], one set of launches for the band.
 * bldp_kurtosis_blocks_host_f32: host in, host (nc, ni, nb) out; the window's
 * rows are staged on device `dev`.  Synchronous. */
BLDP_API int bldp_kurtosis_blocks_shape(int64_t nchan, int64_t nif, int64_t ntime,
                                        const int64_t *win, int64_t tblock, int64_t dims[3]);
BLDP_API int bldp_kurtosis_blocks_plan_f32(const float *in, int64_t nchan, int64_t nif,
                                           int64_t ntime, const int64_t *win, int64_t tblock,
                                           int64_t info[4]);
BLDP_API int bldp_kurtosis_blocks_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                      const int64_t *win, int64_t tblock, double *out,
                                      int64_t out_ld_i, int64_t out_ld_b, void *stream);
BLDP_API int bldp_band_kurtosis_blocks_f32(int nbank, const float *const *in, int64_t nchan,
                                           int64_t nif, int64_t ntime, const int64_t *win,
                                           int64_t tblock, double *out, void *stream);
BLDP_API int bldp_kurtosis_blocks_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                           int64_t ntime, const int64_t *win, int64_t tblock,
                                           double *out);

/* Skewness over time of every (channel, if) row of the window (getskewness:
 * StatsBase.skewness where getkurtosis maps StatsBase.kurtosis), Float64:
 *   m = mean(v) (Float32, Base.sum's pairwise sum / n, the kurtosis' m)
 *   z = v[i] - m, z2 = z * z (Float32); cm2 += z2; cm3 += z2 * z (a Float32
 *   product; Float64 sums); (cm3 / n) / sqrt((cm2/n) * (cm2/n) * (cm2/n))
 * n = 1 and constant rows give NaN.  One family covers the whole window and
 * blocks of spectra: tblock = 0 is the whole window (nb = 1, the planner of
 * bldp_kurtosis_f32), tblock >= 1 cuts the selected spectra into nb = nt /
 * tblock blocks as bldp_kurtosis_blocks_f32 does (its planner, its one-launch
 * forms, block by block otherwise) and element (c, i, b) is the rule applied
 * to block b alone.  tblock < 0 is BLDP_EINVAL, a tblock that does not divide
 * nt BLDP_EDIM, a window outside the array BLDP_EBOUNDS, a null in / out for
 * a non-empty result BLDP_EINVAL.  The result has the shape
 * bldp_kurtosis_blocks_shape gives (nb = 1 for tblock = 0).  Paths and
 * classes are the kurtosis': <= 32 spectra bit-identical to the rule, the
 * register tile and the two-pass path the rule's terms in another order, the
 * streamed leaves exact z^2 and z^3 in Float64.  Scratch is leased from the
 * library; bldp_kurtosis_workspace_size bounds it.  Additive in ABI 5.
 *
 * bldp_skewness_plan_f32: info = {path (as bldp_kurtosis_plan_f32), 1 = one
 * launch set / 0 = block by block, nb, workspace bytes}; launches nothing and
 * needs no GPU.
 * bldp_skewness_f32: element (c, i, b) at out[c + i*out_ld_i + b*out_ld_b]
 * (elements; out_ld_b is not read for tblock = 0).  Asynchronous.
 * bldp_band_skewness_f32: in[] is a HOST array of device pointers; out is
 * dense [nbank][nb][ni][nc], one set of launches for the band.
 * bldp_skewness_host_f32: host in, host (nc, ni, nb) out; the window's rows
 * are staged on device `dev`.  Synchronous. */
BLDP_API int bldp_skewness_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                    const int64_t *win, int64_t tblock, int64_t info[4]);
BLDP_API int bldp_skewness_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                               const int64_t *win, int64_t tblock, double *out, int64_t out_ld_i,
                               int64_t out_ld_b, void *stream);
BLDP_API int bldp_band_skewness_f32(int nbank, const float *const *in, int64_t nchan,
                                    int64_t nif, int64_t ntime, const int64_t *win,
                                    int64_t tblock, double *out, void *stream);
BLDP_API int bldp_skewness_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int64_t tblock,
                                    double *out);

/* Mean, variance, skewness and kurtosis of every (channel, if) row of the
 * window from one read of it (getmoments): what bldp_kurtosis_f32 and
 * bldp_skewness_f32 give, with the two numbers both already form, as up to
 * four Float64 planes.  Over the n selected spectra of a row, or of each block
 * of tblock spectra:
 *   m = mean(v) (Float32, Base.sum's pairwise sum / n, the kurtosis' m)
 *   z = v[i] - m, z2 = z * z (Float32); cm2 += z2; cm3 += z2 * z;
 *   cm4 += z2 * z2 (Float32 products, Float64 sums, index order)
 *   mean = Float64(m);  var = cm2 / n;
 *   skewness = (cm3 / n) / sqrt((cm2 / n)^3);  kurtosis = (cm4 / n) / (cm2 / n)^2 - 3
 * var is the UNCORRECTED variance cm2 / n that both StatsBase recipes divide
 * by, not Julia's var (which divides by n - 1).  n = 0 gives NaN in every
 * plane.  tblock, the shape, the planner, the paths and their classes are
 * bldp_skewness_f32's; the skewness and kurtosis planes hold the bits
 * bldp_skewness_f32 and bldp_kurtosis_f32 (bldp_kurtosis_blocks_f32) give for
 * the same call, except that plans which take bldp_kurtosis_f32 to its
 * register-tile leaf kernel (plan option "kurt_leaf_tile") compare with that
 * option at 0.  The four planes share their strides; any of them may be NULL
 * and is then neither formed in memory nor stored.  Errors: tblock < 0
 * BLDP_EINVAL, a tblock that does not divide nt BLDP_EDIM, a window outside
 * the array BLDP_EBOUNDS, and for a non-empty result BLDP_EINVAL for a null
 * in, for four NULL planes, and for planes that overlap each other or the
 * input array.  Scratch is leased from the library.  Additive in ABI 5.
 *
 * bldp_moments_plan_f32: info = {path, 1 = one launch set / 0 = block by
 * block, nb, workspace bytes} as bldp_skewness_plan_f32 (the workspace differs
 * where the two-pass path keeps a third partial sum per chunk and where the
 * block-by-block form stages four planes); launches nothing, needs no GPU.
 * bldp_moments_f32: element (c, i, b) at plane[c + i*out_ld_i + b*out_ld_b]
 * (elements; out_ld_b is not read for tblock = 0).  Asynchronous.
 * bldp_band_moments_f32: in[] is a HOST array of device pointers; each plane
 * is dense [nbank][nb][ni][nc], one set of launches for the band.
 * bldp_moments_host_f32: host in, host (nc, ni, nb) planes out; the window's
 * rows are staged on device `dev` once.  Synchronous. */
BLDP_API int bldp_moments_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                   const int64_t *win, int64_t tblock, int64_t info[4]);
BLDP_API int bldp_moments_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                              const int64_t *win, int64_t tblock, double *mean, double *var,
                              double *skew, double *kurt, int64_t out_ld_i, int64_t out_ld_b,
                              void *stream);
BLDP_API int bldp_band_moments_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                   int64_t ntime, const int64_t *win, int64_t tblock,
                                   double *mean, double *var, double *skew, double *kurt,
                                   void *stream);
BLDP_API int bldp_moments_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                   int64_t ntime, const int64_t *win, int64_t tblock,
                                   double *mean, double *var, double *skew, double *kurt);

/* Statistics over blocks of spectra (getdata(...; tavby, tavfunc)): fqav's rule
 * on the time axis with Julia's Statistics as the function.  The window's
 * selected spectra are cut into nb = nt / tavby blocks, block b holding spectra
 * [b*tavby, (b+1)*tavby), and element (c, i, b) of the (nc, ni, nb) Float32
 * result is op of that block of column (c, i): BLDP_OP_VAR (the corrected
 * variance about the mean), BLDP_OP_STD (its root) or BLDP_OP_MEDIAN (ordered
 * by isless, the middle element of an odd block, a/2 + b/2 in Float32 of an
 * even one, NaN when the block holds a NaN) or BLDP_OP_MAD (the normalised
 * median absolute deviation of enum bldp_op: the median of |x - median| by the
 * same rule, times 1.4826022185056018 in Float64, rounded to Float32).  A
 * constant block gives exactly
 * +0.0 for var / std / mad.  Any other op is BLDP_EINVAL (sum / mean / max / min over
 * time are bldp_reduce_* with tavby); a tavby that does not divide nt is
 * BLDP_EDIM, a window outside the array BLDP_EBOUNDS.  tavby <= 1 copies the
 * window (fqav's n <= 1 rule, as bldp_reduce_f32 with fqavby = tavby = 1).
 * Additive in ABI 5.
 *
 * Blocks of <= 32 spectra are held in registers, one lane per column (four
 * columns with float4 loads: unit channel step, nc a multiple of 4); longer
 * blocks are split over the time slices of a workgroup that meet through LDS,
 * var / std in two passes with Float64 accumulators, the median by an 8-bit
 * radix select that re-reads the block every pass.  mad runs the median's
 * selection twice in the same kernel (the register form on its registers, the
 * split form re-reading the block and forming |x - median| on the fly) and
 * reports the median's path with passes = 2 (registers), 8 (split, odd tavby)
 * or 10 (split, even tavby).  One launch, no workspace;
 * var / std of blocks too few to fill the GPU are also cut into time chunks
 * across workgroups (three launches, Float64 partials in library scratch leased
 * for the call, added in a fixed order).
 *
 * bldp_tstat_shape: dims = {nc, ni, nb}; pure host, every argument check but
 * the op's.
 * bldp_tstat_plan_f32: info = {path (0 regs_moments, 1 regs_median,
 * 2 split_moments, 3 split_median, 4 chunk_moments; -1 the copy of tavby <= 1), channels per
 * lane, time slices of a workgroup splitting a block, passes over the block,
 * workgroups per bank, workspace bytes, nb, lanes along the channels of a split
 * workgroup}; launches nothing and needs no GPU (pointers may be null).
 * bldp_tstat_f32: device pointers, asynchronous on `stream`; element (c, i, b)
 * at out[c + i*out_ld_i + b*out_ld_b] (elements; dense = (nc, nc*ni)), so a
 * bank can write its slot of a stitched product.
 * bldp_band_tstat_f32: in[] is a HOST array of device pointers of banks with
 * one geometry; out is the vcat of the banks, dense (nbank*nc, ni, nb); one
 * launch for the band.
 * bldp_tstat_host_f32: host in, host dense (nc, ni, nb) out; the window's rows
 * are staged on device `dev`.  Synchronous. */
BLDP_API int bldp_tstat_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                              int64_t tavby, int64_t dims[3]);
BLDP_API int bldp_tstat_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                 const int64_t *win, int64_t tavby, int op, const float *out,
                                 int64_t info[8]);
BLDP_API int bldp_tstat_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                            const int64_t *win, int64_t tavby, int op, float *out,
                            int64_t out_ld_i, int64_t out_ld_b, void *stream);
BLDP_API int bldp_band_tstat_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                 int64_t ntime, const int64_t *win, int64_t tavby, int op,
                                 float *out, void *stream);
BLDP_API int bldp_tstat_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                 int64_t ntime, const int64_t *win, int64_t tavby, int op,
                                 float *out);

/* quantile(p): Statistics.quantile(x, p) (Julia's default, type 7, alpha = beta
 * = 1) of every block of n channels (axis = 0: fqavfunc, the blocks and the
 * output of bldp_reduce_* with fqavby = n, tavby <= 1) or of n spectra (axis =
 * 2: tavfunc, the blocks and the output of bldp_tstat_*) of a Float32 window.
 * The entry points carrying `int op` have no room for p, so quantile has this
 * family of its own and is no value of enum bldp_op.  Additive in ABI 5.
 *
 * The rule, for a block x of n >= 2 values and a Float64 p in [0, 1]:
 *  1. v[1..n] = x ordered by isless (-0.0 < 0.0, -Inf lowest, +Inf highest);
 *  2. in Float64, every operation rounded once (never fused):
 *     m = 1 + p * (1 - 1 - 1), aleph = n * p + m,
 *     j = clamp(trunc(aleph), 1, n - 1), g = clamp(aleph - j, 0, 1);
 *  3. a = v[j], b = v[j + 1] (the second is always taken, also when g == 0);
 *  4. a and b both finite: d = b - a rounded once to Float32,
 *     r = Float64(a) + g * Float64(d), a Float64 product then a Float64 sum;
 *  5. otherwise r = (1 - g) * Float64(a) + g * Float64(b), not fused either:
 *     g == 0 next to an infinite b, or g == 1 next to an infinite a, is NaN
 *     (0 * Inf), the formula as it stands;
 *  6. the result is Float32(r);
 *  7. a block holding a NaN gives NaN (Julia throws; a kernel cannot, and the
 *     median's "NaN wins" applies);
 *  8. n <= 1 copies the window, as fqav does for every function.
 * quantile(0.5) of an even block is a + 0.5 (b - a), not the median's
 * middle(a, b) = a/2 + b/2: the two may differ in the last bit.
 *
 * The kernels, plans and limits are the median's of the same axis and shape (a
 * quantile selects ranks j - 1 and j, 0-based, where the median selects
 * (n-1)/2 and n/2); the time axis' split form always makes its fifth pass.
 * p outside [0, 1] or NaN, or an axis other than 0 and 2, is BLDP_EINVAL; an n
 * that does not divide the axis is BLDP_EDIM, a window outside the array
 * BLDP_EBOUNDS; all before any launch.
 *
 * bldp_quantile_shape: dims = {nc / n, ni, nt} (axis 0) or {nc, ni, nt / n}
 * (axis 2); pure host.
 * bldp_quantile_plan_f32: info as the median's plan of that axis reports it
 * (axis 0: bldp_reduce_plan_f32, axis 2: bldp_tstat_plan_f32), except that the
 * workspace-bytes slot, which the median never uses (info[6] on axis 0,
 * info[5] on axis 2), carries the 0-based lower rank j - 1 (-1 for the copy of
 * n <= 1).  Launches nothing and needs no GPU (pointers may be null).
 * bldp_quantile_f32: device pointers, asynchronous on `stream`; output element
 * (c, i, t) at out[c + i*out_ld_i + t*out_ld_t] (elements).
 * bldp_band_quantile_f32: in[] is a HOST array of device pointers of banks with
 * one geometry; out is laid out as bldp_band_reduce_f32's (axis 0) or
 * bldp_band_tstat_f32's (axis 2); one launch for the band.
 * bldp_quantile_host_f32: host in, host dense out (the dims of
 * bldp_quantile_shape); the window's rows are staged on device `dev`.
 * Synchronous. */
BLDP_API int bldp_quantile_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                                 int axis, int64_t n, int64_t dims[3]);
BLDP_API int bldp_quantile_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                    const int64_t *win, int axis, int64_t n, double p,
                                    const float *out, int64_t info[8]);
BLDP_API int bldp_quantile_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                               const int64_t *win, int axis, int64_t n, double p, float *out,
                               int64_t out_ld_i, int64_t out_ld_t, void *stream);
BLDP_API int bldp_band_quantile_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int axis, int64_t n,
                                    double p, float *out, void *stream);
BLDP_API int bldp_quantile_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int axis, int64_t n,
                                    double p, float *out);

/* quantiles(ps): np quantiles of every block from ONE read and one selection,
 * Julia's vector form quantile(v, [p1, ..., pK]).  The result is np planes;
 * plane k is, bit for bit, what bldp_quantile_* returns for p[k] on the same
 * window: rules 1 to 8 above applied per plane, NaN wins in every plane, and
 * n <= 1 copies the window into every plane.  In Julia terms
 * stack([fqav(A, n; f = x -> quantile(x, p)) for p in ps]) with the new axis
 * last.  The planes are in the caller's order: p[] may be unsorted and may
 * repeat.  Additive in ABI 5.
 *
 * The host turns (n, p[]) into the sorted distinct 0-based ranks {j_k - 1, j_k}
 * (at most 2 np) and, per plane, which two of them it joins with which weight
 * g_k; the kernels select the keys of those ranks once and write every plane.
 * The median's kernels of that axis and shape do it:
 *   axis 0, n <= 64 and axis 2, n <= 32: one sort in registers, then a pick and
 *     a store per plane (1 read of the block);
 *   axis 0, 64 < n <= 4096: the radix select of all ranks in the same four
 *     passes over keys loaded once (1 read); ranks whose fixed prefixes agree
 *     share a 256-bin histogram, at most 16 of them (16 KiB of LDS);
 *   axis 0, n > 4096: the same, the block read once per pass (4 reads, not
 *     4 np);
 *   axis 2, n > 32: pass 0 builds one histogram per column for all ranks; then
 *     the distinct lower ranks j_k - 1 go three per sweep of passes 1 to 3 and
 *     a pass for the smallest key above each (the upper rank is the same key
 *     again or that one), 16 columns a workgroup (48 KiB of LDS; one lower
 *     rank: 32 columns, 32 KiB, the quantile's own tiling).  Reads of the
 *     block: 1 + 4 ceil(L / 3) for L distinct lower ranks, that is 5, 5, 5, 9,
 *     9, 9, 13, 13 for L = 1 .. 8, where np separate calls read it 5 np times.
 *
 * One launch takes 1 <= np <= BLDP_MAX_QUANTILES probabilities; callers with
 * more batch them.  np outside that, any p[k] outside [0, 1] or NaN, a null p
 * or an axis other than 0 and 2 is BLDP_EINVAL; an n that does not divide the
 * axis is BLDP_EDIM, a window outside the array BLDP_EBOUNDS; all before any
 * launch.
 *
 * bldp_quantiles_shape: dims = {nc / n, ni, nt, np} (axis 0) or {nc, ni,
 * nt / n, np} (axis 2); pure host.
 * bldp_quantiles_plan_f32: info[0..7] as the median's plan of that axis and
 * shape reports it (axis 0: bldp_reduce_plan_f32; axis 2: bldp_tstat_plan_f32,
 * with the passes, workgroups and channel lanes of the tiling above),
 * info[8] = the count of distinct ranks (0 for the copy of n <= 1), info[9] =
 * the reads of the block.  Launches nothing and needs no GPU (pointers may be
 * null).
 * bldp_quantiles_f32: device pointers, asynchronous on `stream`; element (c, i,
 * t) of plane k at out[c + i*out_ld_i + t*out_ld_t + k*out_ld_q] (elements;
 * planes must not overlap: BLDP_EINVAL).
 * bldp_band_quantiles_f32: as bldp_band_quantile_f32, np dense planes of the
 * stitched product one after the other.
 * bldp_quantiles_host_f32: host in, host dense out (the dims of
 * bldp_quantiles_shape, plane k at k * dims[0]*dims[1]*dims[2]); the window's
 * rows are staged on device `dev` once.  Synchronous. */
#define BLDP_MAX_QUANTILES 8
BLDP_API int bldp_quantiles_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                                  int axis, int64_t n, int np, int64_t dims[4]);
BLDP_API int bldp_quantiles_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                     const int64_t *win, int axis, int64_t n, int np,
                                     const double *p, const float *out, int64_t info[10]);
BLDP_API int bldp_quantiles_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                const int64_t *win, int axis, int64_t n, int np, const double *p,
                                float *out, int64_t out_ld_i, int64_t out_ld_t, int64_t out_ld_q,
                                void *stream);
BLDP_API int bldp_band_quantiles_f32(int nbank, const float *const *in, int64_t nchan,
                                     int64_t nif, int64_t ntime, const int64_t *win, int axis,
                                     int64_t n, int np, const double *p, float *out,
                                     void *stream);
BLDP_API int bldp_quantiles_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                     int64_t ntime, const int64_t *win, int axis, int64_t n,
                                     int np, const double *p, float *out);

/* outliers: the median, the mad, the count of outliers and the outlier flags of
 * every block from ONE launch.  Blocks, windows and geometry are those of
 * bldp_quantile_*: n selected channels (axis 0) or n selected spectra (axis 2),
 * n >= 2.  Additive in ABI 5.  For a block x[0 .. n-1]:
 *  1. c = median(x): BLDP_OP_MEDIAN's bits.
 *  2. d_i = |x_i - c|, the difference rounded once to Float32.
 *  3. s = Float32(Float64(median(d)) * 1.4826022185056018): BLDP_OP_MAD's bits.
 *  4. thr = Float32(nsigma * Float64(s)): one Float64 product, rounded once.
 *  5. Sample i is flagged when d_i > thr, a strict Float32 compare: d_i == thr
 *     is not flagged, s == 0 flags exactly the samples that differ from the
 *     median, thr == +Inf flags nothing (nor does the NaN of 0 * Inf).
 *  6. A NaN c or s flags nothing (a block holding a NaN, Inf - Inf deviations).
 *  7. count = the flagged samples of the block (uint32).
 *  8. mask[i] = 1 for a flagged sample, else 0 (uint8, dense over the window).
 * Only this two-sided test exists.
 *
 * The median's kernels of that axis and shape do it, as mad's two selections
 * and then one compare per element.  Reads of the block (info[8]):
 *   axis 0, n <= 4096 and axis 2, n <= 32 (the block's keys in registers): 1
 *     without a mask, 2 with one (the mask pass reads the block again for the
 *     positions);
 *   axis 0, n > 4096: 9 (mad's 8 and the flag pass);
 *   axis 2, n > 32: mad's 8 (odd n) or 10 (even n), and 1.
 *
 * nsigma negative, NaN or infinite, n < 2 or an axis other than 0 and 2 is
 * BLDP_EINVAL; an n that does not divide the axis is BLDP_EDIM, a window
 * outside the array BLDP_EBOUNDS; so are (BLDP_EINVAL) four null outputs of a
 * non-empty result and outputs that overlap each other or the input; all
 * before any launch.
 *
 * bldp_outliers_shape: dims = bldp_quantile_shape's, mask_dims = the window's
 * {nc, ni, nt}; pure host.
 * bldp_outliers_plan_f32: info[0..7] as mad's plan of that axis and shape
 * reports it (axis 0: bldp_reduce_plan_f32 with BLDP_OP_MAD; axis 2:
 * bldp_tstat_plan_f32), info[8] = the reads of the block, info[9] = 1 when a
 * mask is written, else 0.  Launches nothing and needs no GPU (the pointer may
 * be null).
 * bldp_outliers_f32: device pointers, asynchronous on `stream`, one launch, no
 * workspace.  Element (c', i, t') of med, mad and count at [c' + i*out_ld_i +
 * t'*out_ld_t] (elements); mask is the dense (nc, ni, nt) window, element (c, i,
 * t) at mask[c + nc*(i + ni*t)].  Any output may be NULL and is then neither
 * formed nor stored.
 * bldp_band_outliers_f32: one launch for nbank banks; med, mad and count are
 * laid out as bldp_band_quantile_f32's product, mask is the vcat of the banks'
 * windows, (nbank*nc, ni, nt).
 * bldp_outliers_host_f32: host in, host dense outs (any may be NULL); the
 * window's rows are staged on device `dev` once.  Synchronous. */
BLDP_API int bldp_outliers_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                                 int axis, int64_t n, int64_t dims[3], int64_t mask_dims[3]);
BLDP_API int bldp_outliers_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                    const int64_t *win, int axis, int64_t n, int want_mask,
                                    int64_t info[10]);
BLDP_API int bldp_outliers_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                               const int64_t *win, int axis, int64_t n, double nsigma, float *med,
                               float *mad, uint32_t *count, uint8_t *mask, int64_t out_ld_i,
                               int64_t out_ld_t, void *stream);
BLDP_API int bldp_band_outliers_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int axis, int64_t n,
                                    double nsigma, float *med, float *mad, uint32_t *count,
                                    uint8_t *mask, void *stream);
BLDP_API int bldp_outliers_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                    int64_t ntime, const int64_t *win, int axis, int64_t n,
                                    double nsigma, float *med, float *mad, uint32_t *count,
                                    uint8_t *mask);

/* fqavfunc argmax / argmin (fqav(A, n; f=argmax), the position half of Julia's
 * findmax / findmin): where in each block of the reduce the extreme lies.  For
 * output element (c', i, t') the block is the F x T selected elements
 * bldp_reduce_f32 takes (F = fqavby channels by T = tavby spectra, after the
 * window's offsets, steps and direction), numbered off = k + F * tt, 0-based,
 * k along the selected channels and tt along the selected spectra: column-major,
 * the order of reshape(A, (F, :, ni, T, :)).
 *   BLDP_ARG_MAX  a block holding a NaN gives the smallest off of a NaN (any
 *                 sign or payload); otherwise the smallest off among the
 *                 elements greatest under isless (-0.0 < 0.0, +Inf highest).
 *   BLDP_ARG_MIN  NaN wins the same way; otherwise the smallest off among the
 *                 isless-least elements (of (0.0, -0.0) the -0.0).
 * idx receives off (< 2^31, so the buffer may be read as int32); val, when not
 * NULL, the bit pattern of the winning element, copied (a NaN result carries the
 * first NaN's payload).  The result does not depend on how the launch divides a
 * block.  fqavby <= 1 and tavby <= 1 (blocks of one element) give index 0 and
 * the window itself.  Divisibility, window and bounds rules are those of
 * bldp_reduce_f32 (BLDP_EDIM, BLDP_EBOUNDS; the output shape is
 * bldp_reduce_shape's); F * T > 2^31 - 1, an argop other than the two, a null
 * in / idx for a non-empty result, and idx / val overlapping the input or each
 * other are BLDP_EINVAL.  An empty result launches nothing.  Float32 input;
 * additive in ABI 5.
 *
 * Blocks of F <= 1024 are shared by the 1 .. 64 lanes of a wave that stream the
 * T rows (path 0, "lanes"); with long T and too few outputs to fill the GPU the
 * rows are split over the time slices of a workgroup that meet through LDS
 * (path 1, "lanes_tsplit"); F > 1024 takes one workgroup per block (path 2,
 * "block").  One launch, no workspace; chunks of T across workgroups are not
 * built.
 *
 * bldp_argext_plan_f32: info = {path, lanes per block (256 = a workgroup), time
 * slices, float4 loads per lane per row (0: one dword per element), workgroups
 * per bank, workspace bytes (0), outputs per bank, vector loads 1 / 0}; launches
 * nothing and needs no GPU (pointers may be null).
 * bldp_argext_f32: device pointers, asynchronous on `stream`; element
 * (c', i, t') of both outputs at [c' + out_ld_i * i + out_ld_t * t'].
 * bldp_band_argext_f32: in[] is a HOST array of device pointers of banks with
 * one geometry; idx / val are dense (nbank*nco, ni, nto), the vcat of the banks
 * (offsets are relative to each block, so stitching is concatenation); one launch.
 * bldp_argext_host_f32: host in, host dense (nco, ni, nto) out; the window's
 * rows are staged on device `dev`.  Synchronous. */
enum bldp_argop { BLDP_ARG_MAX = 0, BLDP_ARG_MIN = 1 };
BLDP_API int bldp_argext_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                  const int64_t *win, int64_t fqavby, int64_t tavby, int argop,
                                  const uint32_t *idx, int64_t info[8]);
BLDP_API int bldp_argext_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                             const int64_t *win, int64_t fqavby, int64_t tavby, int argop,
                             uint32_t *idx, float *val, int64_t out_ld_i, int64_t out_ld_t,
                             void *stream);
BLDP_API int bldp_band_argext_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, int64_t fqavby,
                                  int64_t tavby, int argop, uint32_t *idx, float *val,
                                  void *stream);
BLDP_API int bldp_argext_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, int64_t fqavby,
                                  int64_t tavby, int argop, uint32_t *idx, float *val);

/* Masked reduce: integrate a window over its unflagged samples.  One read of the
 * window and one read of a byte mask give, for every fqavby x tavby block of the
 * reduce, the sum (or mean) of the unflagged samples and how many there were;
 * the kept count is the weight that any later averaging of the products needs.
 * Float32 input; additive in ABI 5.
 *
 * The block of output (c', i, t') is the reduce's.  It is the F = fqavby selected
 * channels by T = tavby selected spectra that bldp_reduce_f32 takes, after the
 * window's offsets, steps and direction.
 *
 * The mask is addressed in window coordinates, like the one bldp_outliers_f32
 * writes.  Flag (c, i, t) of the selected (nc, ni, nt) window is the byte
 * mask[c*mask_ld[0] + i*mask_ld[1] + t*mask_ld[2]].
 *  - mask_ld == NULL means dense: {1, nc, nc*ni}.  The "mask" of outliers goes
 *    in as it is.
 *  - A stride of 0 broadcasts along that axis.  A bad-channel list is {1, 0, 0};
 *    a bad-spectrum list is {0, 0, 1}.
 *  - Negative strides are BLDP_EINVAL.
 *
 * The steps are:
 *  1. A sample is kept when its byte is 0 and flagged for any other value: 1, 2,
 *     255.
 *  2. kept (uint32) is the number of kept samples of the block.
 *  3. sum (BLDP_OP_SUM) is the Float32 sum of the kept samples, in any order, as
 *     the plain reduce leaves its order open.  A flagged sample is excluded by
 *     selection, never multiplied by 0: a flagged NaN or +-Inf leaves the result
 *     finite, and a kept NaN propagates.  A block with nothing kept gives 0.0,
 *     Julia's sum(Float32[]).
 *  4. mean (BLDP_OP_MEAN) is that sum divided once by Float32(kept).  It is a
 *     correctly rounded IEEE division (the kernels use __fdiv_rn).  Nothing kept
 *     gives NaN (0/0), Julia's mean(Float32[]).
 *  5. Every other op is BLDP_EINVAL.
 *  6. Before any launch, each of the following is refused with the codes the
 *     sibling entry points use: F*T > 2^31 - 1 (Python and the shim read Int32);
 *     both outputs null on a non-empty result; a null mask; outputs that overlap
 *     each other, the input window or the mask's span; output strides that
 *     overlap (all BLDP_EINVAL); factors that do not divide the window
 *     (BLDP_EDIM); a window outside the array (BLDP_EBOUNDS).
 *  7. F = T = 1 is legal: data = kept ? x : 0.
 *
 * The walk of a block is bldp_argext_*'s, with the same three paths ("lanes",
 * "lanes_tsplit", "block") chosen by the same plan.  The flags are loaded as one
 * aligned dword for the four flags of a float4 (float4 data loads, mask_ld[0] ==
 * 1, the mask pointer a multiple of 4 and every non-zero mask pitch a multiple
 * of 4), as one byte per row when mask_ld[0] == 0, else as one byte per element.
 * One launch, no workspace, no atomics.  The output shape is bldp_reduce_shape's.
 *
 * bldp_masked_reduce_plan_f32: info[0..7] as bldp_argext_plan_f32 reports them
 * {path, lanes per block, time slices, float4 loads per lane per row, workgroups
 * per bank, workspace bytes (0), outputs per bank, vector loads 1 / 0}, info[8]
 * the mask load form (0 byte, 1 dword, 2 row-uniform), info[9] reserved (0).
 * Launches nothing and needs no GPU; both pointers may be null (their alignment
 * only chooses the load width, and a null pointer counts as aligned).
 * bldp_masked_reduce_f32: device pointers, asynchronous on `stream`, one launch;
 * element (c', i, t') of out and kept at [c' + out_ld_i * i + out_ld_t * t'].
 * out or kept may be NULL (not both) and is then neither formed nor stored.
 * bldp_band_masked_reduce_f32: in[] is a HOST array of device pointers of banks
 * with one geometry; one launch; out / kept are dense (nbank*nco, ni, nto), the
 * vcat product of bldp_band_argext_f32.  Bank b's channel c is channel b*nc + c
 * of the mask; mask_ld == NULL is the dense (nbank*nc, ni, nt) mask that
 * bldp_band_outliers_f32 writes.
 * bldp_masked_reduce_host_f32: host in, host mask (mask_ld in bytes of the host
 * mask), host dense (nco, ni, nto) outs; the window's rows and the mask's span
 * are staged on device `dev` once.  Synchronous. */
BLDP_API int bldp_masked_reduce_plan_f32(const float *in, int64_t nchan, int64_t nif,
                                         int64_t ntime, const int64_t *win, int64_t fqavby,
                                         int64_t tavby, const uint8_t *mask,
                                         const int64_t *mask_ld, int64_t info[10]);
BLDP_API int bldp_masked_reduce_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                    const int64_t *win, int64_t fqavby, int64_t tavby, int op,
                                    const uint8_t *mask, const int64_t *mask_ld, float *out,
                                    uint32_t *kept, int64_t out_ld_i, int64_t out_ld_t,
                                    void *stream);
BLDP_API int bldp_band_masked_reduce_f32(int nbank, const float *const *in, int64_t nchan,
                                         int64_t nif, int64_t ntime, const int64_t *win,
                                         int64_t fqavby, int64_t tavby, int op,
                                         const uint8_t *mask, const int64_t *mask_ld, float *out,
                                         uint32_t *kept, void *stream);
BLDP_API int bldp_masked_reduce_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                         int64_t ntime, const int64_t *win, int64_t fqavby,
                                         int64_t tavby, int op, const uint8_t *mask,
                                         const int64_t *mask_ld, float *out, uint32_t *kept);

/* Histogram: the sample counts per bin of every block.  One streaming read of
 * the window gives, for every fqavby x tavby block of the reduce, how many of its
 * samples fall into each of nbins = B equal bins of [lo, hi), how many lie below
 * and above, and how many are NaN.  Float32 input; additive in ABI 5.
 *
 * The block of output (c', i, t') is the reduce's: F = fqavby selected channels by
 * T = tavby selected spectra, after the window's offsets, steps and direction.
 *
 * Parameters.  Each breach is BLDP_EINVAL with a message and launches nothing:
 *  - 1 <= B <= BLDP_MAX_HIST_BINS;
 *  - lo32 = Float32(lo) and hi32 = Float32(hi) are finite, and lo32 < hi32;
 *  - w = hi32 - lo32 (Float32) is finite;
 *  - s = Float32(B) / w (Float32 division) is finite and above 0;
 *  - F * T <= 2^31 - 1 (Python and the shim read Int32).
 * s is computed on the host, once, and handed to the kernel as a Float32.
 *
 * The rule.  A sample x is classed in this order:
 *  1. x != x: it goes to nan.
 *  2. x < lo32: it goes to below.
 *  3. x >= hi32: it goes to above.
 *  4. Otherwise k = floor((x - lo32) * s) goes to bin min(k, B - 1).
 * The subtraction and the multiplication are two Float32 operations, each rounded
 * once; the rule is not x*s - lo*s.  -Inf is below, +Inf above, and -0.0 with
 * lo = 0 is in bin 0.  A sample is classed before any conversion to an integer,
 * and the index is clamped before it addresses anything.  The clamp is needed:
 * the largest Float32 below hi32 gives k == B for (lo, hi, B) = (-1, 1, 7),
 * (-5, 5, 100) and (-3, 3, 6).  The rule is monotone in x, so every bin is an
 * interval.  Bin k is roughly [lo32 + k*w/B, lo32 + (k+1)*w/B); those edges are
 * a reading aid only, the rule above decides.
 *
 * Output: B + 3 planes of uint32 counts.  Planes 0 .. B-1 are the bins, plane B
 * is below, B + 1 above, B + 2 nan.  Plane q of block (c', i, t') is
 * out[c' + out_ld_i * i + out_ld_t * t' + out_ld_q * q] (the layout of
 * bldp_quantiles_f32).  In every block the planes add up to F * T.  The entry
 * points zero what they need themselves, on the caller's stream: out may hold
 * anything.  Counts are integers, so the result does not depend on how lanes,
 * waves and workgroups share a block, and two calls give identical bits.
 *
 * The paths (info[0]): 0 "block", one workgroup per block; 1 "block_split", a
 * block's rows and columns chunked over several workgroups whose counts are
 * merged by atomic adds into the zeroed output; 2 "lanes", several blocks that are
 * neighbours along the channels share a workgroup, its lanes along the channels;
 * 3 "lanes_tsplit", the same with the time range chunked over workgroups (atomic
 * adds).  Every workgroup counts into LDS and flushes once.  No workspace.
 *
 * bldp_histogram_plan_f32: info = {path, workgroups per bank, chunks per block,
 * blocks per workgroup, LDS bytes, replicas of a block's counters in LDS,
 * workspace bytes (0), vector loads 1 / 0, lanes along the channels, rows per
 * chunk}.  Launches nothing and needs no GPU; the pointer may be null (its
 * alignment only chooses the load width, and a null pointer counts as aligned).
 * bldp_histogram_f32: device pointers, asynchronous on `stream`.
 * bldp_band_histogram_f32: in[] is a HOST array of device pointers of banks with
 * one geometry on one GPU; out is the dense (nbank*nco, ni, nto, B + 3) vcat of
 * the per-bank results.
 * bldp_histogram_host_f32: host in, host dense (nco, ni, nto, B + 3) out; the
 * window's rows are staged on device `dev` once.  Synchronous. */
#define BLDP_MAX_HIST_BINS 4096
BLDP_API int bldp_histogram_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                     const int64_t *win, int64_t fqavby, int64_t tavby,
                                     int nbins, double lo, double hi, int64_t info[10]);
BLDP_API int bldp_histogram_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                const int64_t *win, int64_t fqavby, int64_t tavby, int nbins,
                                double lo, double hi, uint32_t *out, int64_t out_ld_i,
                                int64_t out_ld_t, int64_t out_ld_q, void *stream);
BLDP_API int bldp_band_histogram_f32(int nbank, const float *const *in, int64_t nchan,
                                     int64_t nif, int64_t ntime, const int64_t *win,
                                     int64_t fqavby, int64_t tavby, int nbins, double lo,
                                     double hi, uint32_t *out, void *stream);
BLDP_API int bldp_histogram_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                     int64_t ntime, const int64_t *win, int64_t fqavby,
                                     int64_t tavby, int nbins, double lo, double hi,
                                     uint32_t *out);

/* Hits: the flagged samples of a window as an ordered list, Julia's
 * findall(!iszero, mask) and A[mask] done on the device.  The mask never leaves
 * the device and the result is a short list.  Float32 input; additive in ABI 5.
 *
 * The window is the reduce's: `win` with offsets, steps and direction selects
 * (nc, ni, nt).  The mask is addressed exactly as bldp_masked_reduce_f32
 * addresses it: window coordinates, mask_ld in bytes, NULL = dense {1, nc,
 * nc*ni}, a stride of 0 broadcasts, negative strides are BLDP_EINVAL.  The mask
 * of bldp_outliers_f32 goes in as it is; a bad-channel list is {1, 0, 0}.
 *
 *  1. Sample (c, i, t) is flagged when its byte is not 0 (1, 2, 255): the
 *     complement of the masked reduce's "kept".
 *  2. total (uint64) is the number of flagged samples of the window, always
 *     exact, whatever cap is.
 *  3. The flagged samples are listed in ascending linear window index
 *     k = c + nc*(i + ni*t), Julia's column-major findall order.  idx[j] (int64,
 *     0-based) is the j-th such k, val[j] that sample's Float32 bits, untouched:
 *     a NaN keeps its payload and -0.0 stays -0.0.
 *  4. Only entries j < min(total, cap) are written, the first cap in that order.
 *     Nothing beyond them is touched.
 *  5. idx or val may be NULL and is then not written.  cap = 0 is legal.  With
 *     cap = 0 or both lists NULL the call only counts: the third launch is not
 *     issued.
 *  6. Two calls give identical bytes.  A list position is a function of k and of
 *     integer sums of flag counts alone; no atomic and no arrival order takes
 *     part.
 *  7. Refused before any launch: a null total, a null mask (non-empty window),
 *     cap < 0, outputs that overlap each other, the input window or the mask's
 *     span, more tiles than one launch takes (all BLDP_EINVAL); a window outside
 *     the array (BLDP_EBOUNDS).
 *  8. An empty window gives total = 0 and launches nothing.
 *
 * Band form: the window is the vcat (nbank*nc, ni, nt); bank b's channel c is
 * channel b*nc + c of the mask and of k, as in bldp_band_masked_reduce_f32, so
 * within one (i, t) row all of bank 0 comes before bank 1.
 *
 * The window's linear order is cut into tiles, a contiguous run of k each, one
 * workgroup per tile; three launches on `stream` (count the flags of every
 * tile, one workgroup's exclusive prefix of the counts, write the lists) with
 * 12 bytes of library scratch per tile.  The smallest tile is 4 steps of 256
 * lanes; it doubles until at most 8192 tiles cover the window, up to 2^31
 * elements a tile.  The flags are loaded as one aligned load of 16 or 4 flags a
 * lane (mask_ld[0] == 1, nc a multiple of that width, the mask pointer and
 * every pitch in use a multiple of it), as one byte per row when mask_ld[0] == 0
 * (the count; the list kernel reads that byte per element), else as one byte
 * per element.
 *
 * bldp_hits_plan_f32: info = {mask load form (0 byte, 1 wide, 2 row-uniform),
 * elements per tile, tiles, workspace bytes, chunks the scan workgroup loops
 * over, flags per lane per load, launches (2 for cap = 0, else 3), 0, 0, 0}; all
 * 0 for an empty window.  Launches nothing and needs no GPU; both pointers may
 * be null (a null pointer counts as aligned).
 * bldp_hits_f32: device pointers (total too), asynchronous on `stream`.
 * bldp_band_hits_f32: in[] is a HOST array of device pointers of banks with one
 * geometry; mask_ld == NULL is the dense (nbank*nc, ni, nt) mask.
 * bldp_hits_host_f32: host in, host mask (mask_ld in bytes of the host mask),
 * host lists and total; the window's rows and the mask's span are staged on
 * device `dev` once, the mask is counted twice there (the lists are sized from
 * the first count).  Synchronous. */
BLDP_API int bldp_hits_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                const int64_t *win, const uint8_t *mask, const int64_t *mask_ld,
                                int64_t cap, int64_t info[10]);
BLDP_API int bldp_hits_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, const uint8_t *mask, const int64_t *mask_ld,
                           int64_t cap, int64_t *idx, float *val, uint64_t *total, void *stream);
BLDP_API int bldp_band_hits_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                int64_t ntime, const int64_t *win, const uint8_t *mask,
                                const int64_t *mask_ld, int64_t cap, int64_t *idx, float *val,
                                uint64_t *total, void *stream);
BLDP_API int bldp_hits_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                int64_t ntime, const int64_t *win, const uint8_t *mask,
                                const int64_t *mask_ld, int64_t cap, int64_t *idx, float *val,
                                uint64_t *total);

/* Fold and unfold: a window over its coarse channels.  Every coarse channel of a
 * filterbank product carries the polyphase filterbank's passband; the fold gives
 * that shape as a profile over the fine-channel index, and the unfold takes it out
 * of the window.  Float32 input; additive in ABI 5.
 *
 * The window and its blocks
 *  - win selects (nc, ni, nt) with offsets, steps and direction, as for
 *    bldp_reduce_f32.
 *  - Selected channel c (0-based, in window order) has fine index k = c mod nfpc
 *    and coarse index j = c div nfpc; J = nc / nfpc.
 *  - tavby = T cuts the selected spectra into nto = nt / T blocks; tavby <= 1
 *    means T = 1.
 *  - In Julia terms the fold is
 *    dropdims(sum(reshape(A, nfpc, J, ni, T, nto); dims=(2,4)); dims=(2,4)).
 *
 * Fold, for output (k, i, t').  The block is the J*T samples
 * A[k + nfpc*j, i, t'*T + tt].
 *  1. The mask is optional: mask == NULL keeps everything.
 *  2. The mask is addressed exactly as bldp_masked_reduce_f32 addresses it: in
 *     window coordinates, flag (c, i, t) the byte mask[c*mask_ld[0] + i*mask_ld[1]
 *     + t*mask_ld[2]]; mask_ld == NULL means dense {1, nc, nc*ni}; a stride of 0
 *     broadcasts; a byte of 0 keeps the sample and any other value flags it;
 *     negative strides are BLDP_EINVAL.
 *  3. The mask of bldp_outliers_f32 and a bad-channel list {1, 0, 0} go in as they
 *     are.
 *  4. kept (uint32) is the number of kept samples of the block.
 *  5. BLDP_OP_SUM is the Float64 sum of the kept Float32 samples, in any order,
 *     rounded once to Float32.
 *  6. Blocks reach 64 x 879616 samples on a 0001 bank, so no partial sum is ever
 *     held in Float32: lanes, workgroups and the merge all add Float64.
 *  7. A flagged sample is excluded by selection, never multiplied by 0: a flagged
 *     NaN or +-Inf leaves the result finite, a kept NaN propagates, and a block
 *     with nothing kept gives +0.0.
 *  8. BLDP_OP_MEAN is that Float64 sum divided once in Float64 by Float64(kept),
 *     then rounded once to Float32.  Nothing kept gives NaN.
 *  9. Every other op is BLDP_EINVAL.
 * 10. Two calls give identical bits.  Where a block is shared between workgroups
 *     the Float64 partial sums and the integer counts go to leased library scratch
 *     and a merge launch adds them in an order the plan fixes.  No floating-point atomics.
 *
 * Unfold.  out[c, i, t] = A[c, i, t] o prof[c mod nfpc, i, t div T].
 *  - BLDP_UNFOLD_DIV = 0: one correctly rounded Float32 division; IEEE results
 *    stand for a zero, infinite or NaN profile value.
 *  - BLDP_UNFOLD_SUB = 1: one Float32 subtraction.
 *  - prof is addressed as prof[k + prof_ld_i*i + prof_ld_t*t'], out as
 *    out[c + out_ld_i*i + out_ld_t*t], so a bank can write its slot of a stitched
 *    band.
 *
 * Refusals, all before any launch
 *  - BLDP_EINVAL: nfpc < 1; an op outside the family; J*T > 2^31 - 1 (over all
 *    banks of a band: Python and the shim read Int32 counts); both fold outputs
 *    NULL on a non-empty result; a null in, prof or out; negative mask or profile
 *    strides; negative or overlapping output strides; outputs that overlap each
 *    other, the input window, the mask's span or the profile.  The unfold is
 *    therefore not in place.
 *  - BLDP_EDIM: nfpc not dividing nc, or T not dividing nt.
 *  - BLDP_EBOUNDS: a window outside the array.
 *  - An empty window launches nothing; its shape is (0, ni, nto).
 *
 * Band form, one GPU.  The window is the vcat (nbank*nc, ni, nt); nfpc must divide
 * the per-bank nc, so every bank starts at k = 0.  bldp_band_fold_f32 returns ONE
 * dense (nfpc, ni, nto) profile over all nbank*J coarse channels, not a vcat; bank
 * b's channel c is channel b*nc + c of the mask (mask_ld == NULL: the dense
 * (nbank*nc, ni, nt) mask).  bldp_band_unfold_f32 writes the dense vcat
 * (nbank*nc, ni, nt).
 *
 * The kernels (csrc/fold.hip).  An item is the float4 a lane loads when the channel
 * step is 1, nfpc % 4 == 0 and every row of the window starts on a 16-byte
 * boundary, else one value.  "cols" (more than 128 items per coarse channel): lanes
 * along k, each walking j and tt.  "rows" (up to 128): the lanes of a workgroup lie
 * along c over up to 256 items of a row, several coarse channels, and lanes with
 * equal k meet through LDS.  Where the (k, i, t') tiles alone do not fill the device a block's
 * (bank, j, tt) walk is cut into chunks, a workgroup each, and merged.  The flags
 * are loaded as for the masked reduce: one aligned dword per float4, one byte per
 * row when mask_ld[0] == 0, else a byte per element.
 *
 * bldp_fold_shape: out_shape = (nfpc, ni, nto).
 * bldp_fold_plan_f32: info = {path (0 cols, 1 rows), lanes along the channels,
 * chunks per block, workgroups of the fold launch, workspace bytes, launches (1,
 * or 2 with the merge), mask load form (0 byte, 1 dword, 2 row-uniform, 3 no
 * mask), vector loads 1 / 0, outputs, (bank, coarse group, spectrum) units per
 * chunk}.  Launches nothing and needs no GPU; the pointers may be null (a null
 * pointer counts as aligned).  mask and mask_ld both NULL: no mask; mask NULL and
 * mask_ld given: an aligned mask of those strides.
 * bldp_fold_f32: device pointers, asynchronous on `stream`; out or kept may be
 * NULL (not both) and is then neither formed nor stored.
 * bldp_fold_host_f32: host in, host mask (or NULL), host dense (nfpc, ni, nto)
 * outs; the window's rows and the mask's span are staged on device `dev` once.
 * Synchronous.
 * bldp_unfold_plan_f32: info = {vector loads 1 / 0, workgroups per bank, elements
 * per lane per pass, reserved (0)}.
 * bldp_unfold_f32: device pointers, asynchronous on `stream`, one launch.
 * bldp_unfold_host_f32: host in, host dense (nfpc, ni, nto) prof, host dense
 * (nc, ni, nt) out.  Synchronous. */
enum bldp_unfold_op { BLDP_UNFOLD_DIV = 0, BLDP_UNFOLD_SUB = 1 };
BLDP_API int bldp_fold_shape(int64_t nchan, int64_t nif, int64_t ntime, const int64_t *win,
                             int64_t nfpc, int64_t tavby, int64_t out_shape[3]);
BLDP_API int bldp_fold_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                const int64_t *win, int64_t nfpc, int64_t tavby,
                                const uint8_t *mask, const int64_t *mask_ld, int64_t info[10]);
BLDP_API int bldp_fold_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, int64_t nfpc, int64_t tavby, int op,
                           const uint8_t *mask, const int64_t *mask_ld, float *out,
                           uint32_t *kept, int64_t out_ld_i, int64_t out_ld_t, void *stream);
BLDP_API int bldp_band_fold_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby,
                                int op, const uint8_t *mask, const int64_t *mask_ld, float *out,
                                uint32_t *kept, void *stream);
BLDP_API int bldp_fold_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby,
                                int op, const uint8_t *mask, const int64_t *mask_ld, float *out,
                                uint32_t *kept);
BLDP_API int bldp_unfold_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                  const int64_t *win, int64_t nfpc, int64_t tavby,
                                  const float *prof, int64_t prof_ld_i, int64_t prof_ld_t,
                                  const float *out, int64_t out_ld_i, int64_t out_ld_t,
                                  int64_t info[4]);
BLDP_API int bldp_unfold_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                             const int64_t *win, int64_t nfpc, int64_t tavby, int uop,
                             const float *prof, int64_t prof_ld_i, int64_t prof_ld_t, float *out,
                             int64_t out_ld_i, int64_t out_ld_t, void *stream);
BLDP_API int bldp_band_unfold_f32(int nbank, const float *const *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby,
                                  int uop, const float *prof, int64_t prof_ld_i,
                                  int64_t prof_ld_t, float *out, void *stream);
BLDP_API int bldp_unfold_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                  int64_t ntime, const int64_t *win, int64_t nfpc, int64_t tavby,
                                  int uop, const float *prof, float *out);

/* ---- dedoppler: the drift-rate sums of every channel ------------------------
 * A narrow-band signal that moves d channels while a block of T spectra is
 * recorded is in no single spectrum and not in the sum along a channel; it is in
 * the sum along the sloped path.  Float32 input; additive in ABI 5.
 *
 * The rule, on the selected window W of shape (nc, ni, nt) (after the window's
 * offsets, steps and direction, as every block operation takes it): T = tavby
 * spectra make a block, nb = nt / T; D = maxdrift >= 0 gives K = 2D + 1 drifts
 * d_k = k - D, k = 0 .. 2D, the selected channels moved between the first and the
 * last spectrum of a block.
 *  - Path, in integers: off(d, t) = sign(d) * floor((2|d|t + (T-1)) / (2(T-1))),
 *    the straight line rounded to the nearest channel, halves away from zero.
 *    off(d, 0) = 0, off(d, T-1) = d, off(-d, t) = -off(d, t); two drifts never
 *    share a whole path.  off(5, t) at T = 16: 0 0 1 1 1 2 2 2 3 3 3 4 4 4 5 5.
 *  - Segments: seg > 0 is the number of selected channels of a coarse channel (it
 *    need not divide nc); selected channel c lies in segment c div seg, and a path
 *    takes no sample outside the segment of c.  seg = 0: the whole window is one
 *    segment.  A band is then the vcat of its banks.
 *  - Sum: S[c, i, b, k] = sum over t of W[c + off(d_k, t), i, b*T + t], added in
 *    Float32 in the order t = 0 .. T-1 from +0.0f; a term whose channel lies
 *    outside the segment (or the window) is skipped.  The order is fixed: the
 *    result is a function of the input alone, bit for bit, on any data.
 *  - Best: best[c, i, b] and drift[c, i, b] (the signed d) come from scanning the
 *    drifts in the order 0, -1, +1, -2, +2, ..., -D, +D with BLDP_ARG_MAX's rule:
 *    the first NaN in scan order wins, with its payload; otherwise the first in
 *    scan order among the isless-greatest.  A flat window answers drift = 0.
 *
 * Outputs: best (Float32) and drift (Int32: a C int), (nc, ni, nb), element (c, i, b) at
 * [c + out_ld_i*i + out_ld_t*b]; sums, (nc, ni, nb, K), plane k at + out_ld_q*k
 * (bldp_quantiles_f32's layout).  best and drift go together; that pair or sums
 * may be NULL, not both, and a plane that is not asked for is not written.  sums
 * is for zoom windows: at a whole high-resolution bank (16 spectra) it is K / 16
 * times the input.
 *
 * BLDP_EINVAL: tavby < 2, tavby > 2^20, maxdrift < 0 or > BLDP_MAX_DRIFT (within
 * these the path arithmetic fits 32 bits), seg < 0, outputs that overlap the
 * input window or each other, strides that overlap; BLDP_EDIM: tavby does not
 * divide the selected nt; BLDP_EBOUNDS as in the reduce.  Nothing is launched
 * then.  Every (tavby, maxdrift) inside the caps runs.
 *
 * A workgroup takes a tile of neighbouring channels of one (IF, block), a lane a
 * channel, with the tile's rows and a halo of maxdrift channels on each side in
 * LDS; a lane keeps a group of drifts' sums and its running best in registers and
 * loops over the groups, so best needs no second launch, no atomics and no
 * workspace.  "resident": the block's rows are staged once.  "chunked" (long
 * tavby, or large maxdrift, against the LDS): the rows are staged a chunk at a
 * time and read again for every group.  Both add in the rule's order.
 *
 * bldp_dedoppler_plan_f32: info = {path (0 resident, 1 chunked), channels per
 * tile, halo channels staged on each side, rows per staging chunk, drifts per
 * group, groups, LDS bytes, workgroups per bank, vector loads 1 / 0, workspace
 * bytes (0)}.  Launches nothing and needs no GPU; `in` may be null (a null
 * pointer counts as aligned).
 * bldp_dedoppler_f32: device pointers, asynchronous on `stream`, one launch.
 * bldp_band_dedoppler_f32: host array of device pointers to banks of identical
 * geometry; dense outputs, the vcat of the banks' (bank b's channels at b*nc of
 * every row; sums (nbank*nc, ni, nb, K)); one launch.  Segments are counted from
 * each bank's first selected channel.
 * bldp_dedoppler_host_f32: host in, host dense outs; the window's rows are staged
 * on device `dev` once.  Synchronous. */
#define BLDP_MAX_DRIFT 1024
BLDP_API int bldp_dedoppler_plan_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                     const int64_t *win, int64_t tavby, int64_t maxdrift,
                                     int64_t seg, int64_t info[10]);
BLDP_API int bldp_dedoppler_f32(const float *in, int64_t nchan, int64_t nif, int64_t ntime,
                                const int64_t *win, int64_t tavby, int64_t maxdrift, int64_t seg,
                                float *best, int *drift, float *sums, int64_t out_ld_i,
                                int64_t out_ld_t, int64_t out_ld_q, void *stream);
BLDP_API int bldp_band_dedoppler_f32(int nbank, const float *const *in, int64_t nchan,
                                     int64_t nif, int64_t ntime, const int64_t *win,
                                     int64_t tavby, int64_t maxdrift, int64_t seg, float *best,
                                     int *drift, float *sums, void *stream);
BLDP_API int bldp_dedoppler_host_f32(int dev, const float *in, int64_t nchan, int64_t nif,
                                     int64_t ntime, const int64_t *win, int64_t tavby,
                                     int64_t maxdrift, int64_t seg, float *best, int *drift,
                                     float *sums);

/* Element types other than Float32 (what Blio maps SIGPROC nbits 8 / 16 to, and
 * what HDF5.jl returns for an integer or Float64 dataset: the reference's
 * readers hand any of them to fqav / kurtosis, src/gbtworkerfunctions.jl:173,
 * 181-188, 197-202). */
enum bldp_dtype {
  BLDP_DT_F32 = 0, BLDP_DT_F64 = 1, BLDP_DT_U8 = 2, BLDP_DT_U16 = 3, BLDP_DT_U32 = 4,
  BLDP_DT_U64 = 5, BLDP_DT_I8 = 6, BLDP_DT_I16 = 7, BLDP_DT_I32 = 8, BLDP_DT_I64 = 9
};
/* Element type of fqav's result for input `dtype` and `op`, Julia's:
 *   sum   UInt8/16/32/64 -> UInt64, Int8/16/32/64 -> Int64 (Base.add_sum
 *         widening; exact, wrapping on 64-bit overflow), Float32 / Float64 kept;
 *   mean  Float64 (Float32 kept);  max / min  the input type.
 * Returns the bldp_dtype, or BLDP_EINVAL. */
BLDP_API int bldp_reduce_out_dtype(int dtype, int op);
/* bldp_reduce_strided_f32 for any bldp_dtype: in holds `dtype` elements, out
 * bldp_reduce_out_dtype(dtype, op) elements (strides in elements).  Float32
 * input takes the Float32 kernels; the others one lane per output in the
 * reference's order (integer sums exact).  Device pointers, asynchronous. */
BLDP_API int bldp_reduce_strided(int dtype, const void *in, int64_t nchan, int64_t nif,
                                 int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                                 int op, void *out, int64_t out_ld_i, int64_t out_ld_t,
                                 void *stream);
/* getkurtosis for any bldp_dtype (StatsBase's recipe; Float64 arithmetic for
 * integer and Float64 rows: Base.sum's pairwise Float64 mean, sequential
 * moments; 8- and 16-bit rows from exact integer power sums, within 160 2^-53 of
 * the exactly rounded kurtosis and (3 nt + 175) 2^-53 relative of the
 * recipe on k + 3, plan option "typed_kurt").  out
 * (nc, ni) float64 on the device.  Asynchronous. */
BLDP_API int bldp_kurtosis(int dtype, const void *in, int64_t nchan, int64_t nif, int64_t ntime,
                           const int64_t *win, double *out, void *stream);
/* bldp_reduce_strided / bldp_kurtosis prepared once for fixed buffers (ABI 5;
 * any bldp_dtype, Float32 included): the checks, window and plan are taken
 * here, and each bldp_reduce_launch(handle, stream) only queues the kernel(s)
 * -- what a worker re-reducing the same per-file buffers pays per call
 * (src/gbtworkerfunctions.jl:171-177,191-195).  Same results and errors as
 * the unprepared calls; released with bldp_reduce_release.  Bound to the
 * current device.  bldp_reduce_launch_timed takes these handles too: the
 * Float32 reduce's own dispatches carry the events, the other kinds record
 * them on the stream around the launch. */
BLDP_API int bldp_reduce_prepare(int dtype, const void *in, int64_t nchan, int64_t nif,
                                 int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                                 int op, void *out, int64_t out_ld_i, int64_t out_ld_t,
                                 bldp_reduce_op_t *handle);
BLDP_API int bldp_kurtosis_prepare(int dtype, const void *in, int64_t nchan, int64_t nif,
                                   int64_t ntime, const int64_t *win, double *out,
                                   bldp_reduce_op_t *handle);
/* Host-memory forms (what a Julia worker holding the mmap'ed / read array
 * calls): the window's span is copied to device `dev`, reduced there, and the
 * result copied back into host `out` (dense (nco, ni, nto) of the output type;
 * (nc, ni) float64 for kurtosis).  Synchronous. */
BLDP_API int bldp_reduce_host(int dev, int dtype, const void *in, int64_t nchan, int64_t nif,
                              int64_t ntime, const int64_t *win, int64_t fqavby, int64_t tavby,
                              int op, void *out);
BLDP_API int bldp_kurtosis_host(int dev, int dtype, const void *in, int64_t nchan, int64_t nif,
                                int64_t ntime, const int64_t *win, double *out);

/* HDF5 filter 32008 (bitshuffle + LZ4) chunks, the codec of compressed
 * rawspec FBH5 products (H5Zbitshuffle, reference Project.toml:10; read at
 * src/gbtworkerfunctions.jl:181-187).  A chunk is the raw bytes H5Dread_chunk
 * returns: 12-byte header (uint64 BE uncompressed bytes, uint32 BE block
 * bytes), LZ4 blocks of bit-transposed elements, raw tail of n % 8 elements. */
BLDP_API int bldp_bslz4_info(const void *chunk, size_t nbytes, uint64_t *uncompressed_bytes,
                             uint32_t *block_bytes);
/* Decode one chunk on the host into out (exactly uncompressed_bytes). */
BLDP_API int bldp_bslz4_decode_host(const void *chunk, size_t nbytes, int elem_size, void *out,
                                    size_t out_bytes);
/* Decode nchunk chunks on the GPU.  comp_host and comp_dev hold the same
 * concatenated chunk bytes (the host copy is parsed into a block table, the
 * device copy is decoded); chunk k spans [chunk_off[k], +chunk_len[k]) and
 * decodes to out_dev + out_off[k] (bytes), a slot of out_len[k] bytes: a
 * chunk whose header claims any other size is rejected (BLDP_EINVAL) before
 * anything is launched, so no chunk writes outside its slot.  Synchronous:
 * returns after the decode finished, BLDP_EINVAL if any block is corrupt. */
BLDP_API int bldp_bslz4_decode_dev(int nchunk, const uint8_t *comp_host, const uint8_t *comp_dev,
                                   const uint64_t *chunk_off, const uint64_t *chunk_len,
                                   int elem_size, uint8_t *out_dev, const uint64_t *out_off,
                                   const uint64_t *out_len, void *stream);

/* Asynchronous form: queues the decode on `stream` and returns; error bits
 * are OR-ed into *err_dev (device int, zeroed by the caller before its first
 * call).  The host copy comp_host may be reused once the call returns.
 * bldp_bslz4_error synchronizes `stream` and turns *err_dev into a return
 * code (BLDP_EINVAL for a corrupt block). */
BLDP_API int bldp_bslz4_decode_dev_async(int nchunk, const uint8_t *comp_host,
                                         const uint8_t *comp_dev, const uint64_t *chunk_off,
                                         const uint64_t *chunk_len, int elem_size,
                                         uint8_t *out_dev, const uint64_t *out_off,
                                         const uint64_t *out_len, int *err_dev, void *stream);
BLDP_API int bldp_bslz4_error(const int *err_dev, void *stream);

/* The stored chunks of a chunked FBH5 window, file -> device, natively (the
 * chunk reads and filter 32008 of h5["data"][idxs...],
 * src/gbtworkerfunctions.jl:181-187).  Chunk k (stored_len[k] bytes at
 * file_off[k] of the open file `fd`; 0 bytes = never written) is read with
 * parallel preads (a persistent pool of reader threads per device: 16, or 4
 * fewer than the process's CPU quota when that is less, BLDP_READ_THREADS
 * overrides; they run on the CPUs of the GPU's NUMA node when the caller may
 * use at least half as many CPUs there, and the pinned slots are placed on
 * that node unless the calling thread has a memory policy of its own,
 * BLDP_READ_AFFINITY=0 / BLDP_SLOT_NUMA=0 undo that)
 * into host_pinned + stage_off[k] (both staging buffers hold stage_bytes;
 * dev_out holds out_bytes: every table entry is checked against them before
 * anything is read).  host_pinned NULL (since ABI 4): the reads are staged
 * through the device's library-owned pinned slot ring instead (the one
 * bldp_runs_to_device uses, 8 x 32 MiB; a batch whose staged range is larger
 * takes 2 slots of that size, released when the call returns), batch b in
 * slot b % nslot once that slot's previous copy is done, so pinned host memory
 * stays bounded whatever the window's size: 256 MiB between calls, at most
 * 2 x the largest batch during one; the call then also waits for its last
 * copy before returning.
 * Chunks [batch_end[b-1], batch_end[b]) form
 * batch b: once its reads land, its staged byte range is copied to dev_stage
 * (same offsets) on copy_stream, `stream` waits for that copy, and the batch's
 * chunks are decoded on `stream` into dev_out + k * out_chunk_bytes
 * (bitshuffle + LZ4, bldp_bslz4_decode_dev_async with err_dev; filter_mask
 * bit 0 set = stored without the filter: copied raw; dev_out may be NULL when
 * every chunk is raw: the staged bytes are the output).  Batch b + 1 is read
 * while batch b is copied and decoded.  Returns once every read has landed
 * and every copy and decode is queued; bldp_bslz4_error(err_dev, stream)
 * then synchronizes and reports corrupt blocks.  stats (NULL or 4 doubles):
 * ms to the first queued copy, ms to the last queued work, pread pieces,
 * reader threads. */
BLDP_API int bldp_chunks_to_device(int fd, int64_t nchunk, const int64_t *file_off,
                                   const int64_t *stored_len, const int64_t *stage_off,
                                   const uint32_t *filter_mask, int64_t nbatch,
                                   const int64_t *batch_end, void *host_pinned, void *dev_stage,
                                   int64_t stage_bytes, void *dev_out, int64_t out_chunk_bytes,
                                   int64_t out_bytes, int *err_dev, void *copy_stream,
                                   void *stream, double *stats);

/* bldp_chunks_to_device over the chunks of several files: chunk k is in the
 * open file fd[k] (the banks of a band of compressed FBH5 files read as one
 * stream of batches and decoded into one chunk grid per bank: GBT.getband,
 * src/gbt.jl:69-79,103; src/gbtworkerfunctions.jl:181-187).  Same staging,
 * batches, decode, streams, errors and return as bldp_chunks_to_device (ABI 4). */
BLDP_API int bldp_file_chunks_to_device(int64_t nchunk, const int *fd, const int64_t *file_off,
                                        const int64_t *stored_len, const int64_t *stage_off,
                                        const uint32_t *filter_mask, int64_t nbatch,
                                        const int64_t *batch_end, void *host_pinned,
                                        void *dev_stage, int64_t stage_bytes, void *dev_out,
                                        int64_t out_chunk_bytes, int64_t out_bytes, int *err_dev,
                                        void *copy_stream, void *stream, double *stats);

/* Raw byte runs of a file (an uncompressed contiguous FBH5 `data` dataset or
 * a SIGPROC data block: src/gbtworkerfunctions.jl:171-189) into a dense device
 * block: run r (len[r] bytes at file_off[r]) lands at dev_dst + the sum of
 * the earlier runs' lengths (dev_dst holds dst_bytes).  The block is cut
 * into batches of slot_bytes;
 * the reader threads pread batch b into library-owned pinned slot b % nslot
 * once that slot's previous copy is done, and each batch is copied to the
 * device on copy_stream as soon as its reads land.  Returns after every copy
 * is done; `stream` waits for the last.  stats as bldp_chunks_to_device. */
BLDP_API int bldp_runs_to_device(int fd, int64_t nrun, const int64_t *file_off,
                                 const int64_t *len, void *dev_dst, int64_t dst_bytes,
                                 int64_t slot_bytes, int nslot, void *copy_stream, void *stream,
                                 double *stats);

/* bldp_runs_to_device over runs of several files: run r is in the open file
 * fd[r] (the banks of a band read as one stream of batches into one device
 * block: GBT.getband, src/gbt.jl:69-79,103).  Same batching, slots, streams
 * and return as bldp_runs_to_device. */
BLDP_API int bldp_file_runs_to_device(int64_t nrun, const int *fd, const int64_t *file_off,
                                      const int64_t *len, void *dev_dst, int64_t dst_bytes,
                                      int64_t slot_bytes, int nslot, void *copy_stream,
                                      void *stream, double *stats);

/* Gather a window (Julia order, dense (nc, ni, nt) out) from decoded chunks:
 * packed holds the chunks of a chunk-aligned bounding box back to back in
 * chunk-grid order [gt][gi][gc], each chunk C-order [ct][ci][cc].
 * chunk = {ct, ci, cc}, box0 = {t, i, c} of the box's first element,
 * grid = {gt, gi, gc} chunks in the box, win = the usual 9-int window in
 * dataset coordinates (must lie inside the box). */
BLDP_API int bldp_unchunk_f32(const float *packed, const int64_t chunk[3], const int64_t box0[3],
                              const int64_t grid[3], const int64_t *win, float *out,
                              void *stream);

/* fqav(r::AbstractRange, n): first/step/length of the averaged axis. */
BLDP_API int bldp_fqav_range(double first, double step, int64_t len, int64_t n, double *out_first,
                    double *out_step, int64_t *out_len);

/* Synthetic BL-like filterbank (nchan, nif, ntime) on the device:
 * kind 0 = gamma(2, 5e8) x bandpass scallop x DC spike (nfpc bins per coarse
 * channel); kind 1 = integer-valued 0..255 (order-independent exact sums). */
BLDP_API int bldp_synth_f32(float *out, int64_t nchan, int64_t nif, int64_t ntime, int64_t nfpc,
                   uint64_t seed, int kind, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BLDP_H */
