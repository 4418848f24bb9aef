// Host-side helpers shared by every translation unit that implements include/trpl.h: the thread-local error message, Staged, the
// staging of every host-buffer call (trpl_loglik_multi holds one per shard), the RAII pieces it is made of (CallScope, DevBuf,
// HostPin, HostMap; outside Staged only trpl_loglik_multi_dev uses one, a DevBuf for an sse the caller does not take), LoglikCall,
// the argument record of the fused likelihood, argument checks.  Nothing here throws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <chrono>
#include <type_traits>

#include "../../include/trpl.h"
#include "trpl_common.hpp"

namespace trpl {

// records the message trpl_last_error() returns on this thread and returns `code` (trpl_api.hip)
int api_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return ::trpl::api_fail(TRPL_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

// shard that holds sample s when S samples are cut by trpl_shard_bounds into n_shards ranges: the first
// S % n_shards shards hold one sample more
__host__ __device__ inline int64_t shard_of(int64_t S, int64_t n_shards, int64_t s)
{
    const int64_t base = S / n_shards, rem = S % n_shards, cut = rem * (base + 1);
    return s < cut ? s / (base + 1) : rem + (s - cut) / (base ? base : 1);
}

inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Every host-buffer call works on a private non-blocking stream with stream-ordered allocations, so
// that calls issued from different host threads (or for different devices) overlap on the GPU: nothing
// synchronises the whole device.  Declare the CallScope before the DevBufs of a call: the buffers
// are released (hipFreeAsync) first, then the scope drains and destroys the stream.
struct CallScope {
    hipStream_t st = nullptr;
    hipError_t open() { return hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
    ~CallScope()
    {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
};
struct DevBuf {                      // RAII device allocation for the host-buffer calls
    void *p = nullptr;
    hipStream_t st = nullptr;
    void release() { if (p) (void)hipFreeAsync(p, st); p = nullptr; }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t n, hipStream_t s) { st = s; return hipMallocAsync(&p, n ? n : 1, s); }
    template <typename T> T *as() { return (T *)p; }
};

int select_device(int32_t device);          // hipSetDevice with range check (trpl_api.hip)

// Thresholds (bytes) above which a host-buffer call pins (HostPin) / maps (HostMap) the caller's memory for its duration.
// Measured with environment overrides in round 2 (profiles/r2_dropin_simulate.txt); constants since round 5: the
// library reads no process-wide switch but TRPL_RCCL_LIBRARY.
constexpr long long kHostPinMinBytes = (long long)8 << 20;
constexpr long long kHostDirectMinBytes = (long long)8 << 20;

// The caller's (pageable) host buffer pinned for the duration of a call, so that copies to and from it are
// real asynchronous DMA at PCIe rate instead of being staged through the runtime's bounce buffers.  Pinning
// costs time per page, so only large buffers are worth it; a refused registration (memory that cannot be
// page-locked) is not an error -- the copy then takes the pageable path.  Memory that is already pinned
// (hipHostMalloc, or registered by the caller) is left alone.
// A HostPin / HostMap must outlive the stream's last operation: Staged holds its one before its CallScope.
struct HostPin {
    void *p = nullptr;
    bool pinned = false;
    static bool already_pinned(const void *ptr)
    {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, ptr) == hipSuccess) return at.type == hipMemoryTypeHost;
        (void)hipGetLastError();
        return false;
    }
    void pin(const void *ptr, size_t bytes, unsigned flags = hipHostRegisterDefault)
    {
        constexpr long long min_bytes = kHostPinMinBytes;
        if (!ptr || min_bytes < 0 || bytes < (size_t)min_bytes || already_pinned(ptr)) return;
        if (hipHostRegister((void *)ptr, bytes, flags) == hipSuccess) { p = (void *)ptr; pinned = true; }
        else (void)hipGetLastError();            // clear the sticky error of a refused registration
    }
    ~HostPin() { if (pinned) (void)hipHostUnregister(p); }
};

// The caller's host buffer mapped into the device's address space for the duration of a call: a kernel
// writes its output straight into it across PCIe (no device copy of the matrix, no copy after the kernel).
struct HostMap {
    HostPin pin_;
    // device-visible alias of [ptr, ptr + bytes), or nullptr (too small, refused, switched off)
    void *map(void *ptr, size_t bytes)
    {
        constexpr long long min_bytes = kHostDirectMinBytes;
        if (!ptr || min_bytes < 0 || bytes < (size_t)min_bytes) return nullptr;
        if (!HostPin::already_pinned(ptr)) {
            if (hipHostRegister(ptr, bytes, hipHostRegisterMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            pin_.p = ptr; pin_.pinned = true;
        }
        void *d = nullptr;
        if (hipHostGetDevicePointer(&d, ptr, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return d;
    }
};

// The staging of a host-buffer call around its device-resident (_dev) form: the call declares its buffers, runs the _dev form on
// stream() between begin() and finish(), and returns.  Counts are elements of T (bytes for void); every buffer is compact on the
// device, a pitched one [rows][width] from or to a host leading dimension ld.  The first failed allocation or copy is recorded
// (api_fail, TRPL_ERR_HIP) and turns every later declaration into a no-op that returns NULL; begin() returns it.
// seconds is the device time of the _dev form: from the uploads having landed to its last kernel having finished; a call that
// times its uploads too (open(device, true)) starts the clock once the stream exists.
// Members are destroyed last to first: the buffers are released (hipFreeAsync), then the scope drains and destroys the stream,
// then the caller's memory is unpinned.
struct Staged {
    static constexpr int kMaxBufs = 14;      // the largest user, trpl_loglik_cut_budget off the grid, declares 14 (trpl_loglik_weighted and _cut_levels: 13)
    HostMap hm;                              // the one buffer of the caller's that pin() or map() holds for the call
    CallScope cs;
    DevBuf buf[kMaxBufs];
    struct Back { void *host; const void *dev; size_t ld, width, rows; } back[kMaxBufs];      // in bytes
    int nbuf = 0, nback = 0, rc = TRPL_OK;
    double t0 = 0.0;
    bool timing = false;

    int open(int32_t device, bool clock_from_here = false)
    {
        if (int r = select_device(device)) return r;
        if (ok(cs.open(), "hipStreamCreateWithFlags")) return rc;
        if (clock_from_here) { t0 = now_s(); timing = true; }
        return TRPL_OK;
    }
    hipStream_t stream() const { return cs.st; }
    // The caller's buffer pinned for the copies (HostPin's rules: large and not yet pinned), or mapped for a kernel to write through
    // (HostMap: its device alias, or NULL).  Only on request: in / out / inout never pin.
    void pin(const void *ptr, size_t bytes) { hm.pin_.pin(ptr, bytes); }
    void *map(void *ptr, size_t bytes) { return hm.map(ptr, bytes); }

    int ok(hipError_t e, const char *what)
    {
        if (e != hipSuccess && !rc) rc = api_fail(TRPL_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
        return rc;
    }
    void *scratch(size_t bytes)
    {
        if (rc) return nullptr;
        if (nbuf == kMaxBufs) { rc = api_fail(TRPL_ERR_HIP, "a host-buffer call stages at most %d buffers", kMaxBufs); return nullptr; }
        return ok(buf[nbuf].alloc(bytes, cs.st), "hipMallocAsync") ? nullptr : buf[nbuf++].p;
    }
    // device copy of host[rows][ld], `width` of each row; no copy when host is NULL or there is nothing to copy
    void *up(const void *host, size_t ld, size_t width, size_t rows)
    {
        void *d = scratch(width * rows);
        if (!d || !host || !width || !rows) return d;
        if (rows == 1) ok(hipMemcpyAsync(d, host, width, hipMemcpyHostToDevice, cs.st), "hipMemcpyAsync (upload)");
        else ok(hipMemcpy2DAsync(d, width, host, ld, width, rows, hipMemcpyHostToDevice, cs.st), "hipMemcpy2DAsync (upload)");
        return rc ? nullptr : d;
    }
    // finish() copies d back to host[rows][ld]; not when host is NULL or there is nothing to copy
    void *down(void *d, void *host, size_t ld, size_t width, size_t rows)
    {
        if (d && host && width && rows) back[nback++] = {host, d, ld, width, rows};
        return d;
    }

    template <typename T> const T *in(const T *host, size_t n) { return (const T *)up(host, 0, n * elem<T>(), 1); }
    template <typename T> const T *in(const T *host, size_t ld, size_t width, size_t rows)
    {
        return (const T *)up(host, ld * elem<T>(), width * elem<T>(), rows);
    }
    template <typename T> T *out(T *host, size_t n) { return (T *)down(scratch(n * elem<T>()), host, 0, n * elem<T>(), 1); }
    template <typename T> T *out(T *host, size_t ld, size_t width, size_t rows)
    {
        return (T *)down(scratch(width * elem<T>() * rows), host, ld * elem<T>(), width * elem<T>(), rows);
    }
    template <typename T> T *inout(T *host, size_t n) { return (T *)down(up(host, 0, n * elem<T>(), 1), host, 0, n * elem<T>(), 1); }
    template <typename T> T *inout(T *host, size_t ld, size_t width, size_t rows)
    {
        return (T *)down(up(host, ld * elem<T>(), width * elem<T>(), rows), host, ld * elem<T>(), width * elem<T>(), rows);
    }

    // the first recorded error, else: the uploads have landed, the clock starts unless open() started it
    int begin()
    {
        if (ok(hipStreamSynchronize(cs.st), "hipStreamSynchronize (uploads)")) return rc;
        if (!timing) t0 = now_s();
        return TRPL_OK;
    }
    // the _dev form has finished (*seconds), the outputs are copied back and have landed
    int finish(double *seconds)
    {
        if (ok(hipStreamSynchronize(cs.st), "hipStreamSynchronize")) return rc;
        if (seconds) *seconds = now_s() - t0;
        for (int i = 0; i < nback; i++) {
            const Back &b = back[i];
            if (b.rows == 1) ok(hipMemcpyAsync(b.host, b.dev, b.width, hipMemcpyDeviceToHost, cs.st), "hipMemcpyAsync (download)");
            else ok(hipMemcpy2DAsync(b.host, b.ld, b.dev, b.width, b.width, b.rows, hipMemcpyDeviceToHost, cs.st), "hipMemcpy2DAsync (download)");
        }
        return ok(hipStreamSynchronize(cs.st), "hipStreamSynchronize (downloads)");
    }

private:
    template <typename T> static constexpr size_t elem()
    {
        if constexpr (std::is_void_v<T>) return 1; else return sizeof(T);
    }
};

// Optional profiler ranges (ROCTx) around the host-buffer entry points, so that a marker trace of an UNMODIFIED caller
// (`rocprofv3 --marker-trace --kernel-trace -- python parallel_bayes_gpu.py`) shows the reference's three timed phases
// by name -- pvSim (pvSimPCR.py:378-381), fastlog (probs.py:79-84), prob (probs.py:51-61) -- instead of anonymous kernels
// and copies.  No link dependency (like RCCL): the two symbols are taken from whatever the process already exports
// (rocprofv3 --marker-trace preloads librocprofiler-sdk-roctx.so), else from libroctx64.so if dlopen finds it; absent
// => every range is a no-op (one predictable branch per call).  trpl_api.hip holds the binding.
struct RoctxApi {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
};
const RoctxApi &roctx();
struct ProfRange {
    bool on;
    explicit ProfRange(const char *name) : on(roctx().push != nullptr) { if (on) (void)roctx().push(name); }
    ~ProfRange() { if (on) (void)roctx().pop(); }
    ProfRange(const ProfRange &) = delete;
    ProfRange &operator=(const ProfRange &) = delete;
};

// The arguments of one fused-likelihood call, device pointers: what the trpl_loglik*_dev entry points take, by name.  esum, wts,
// sse_cut (or cut_level) and cut_col select the sink (trpl_loglik_moments / _weighted / _cut / _cut_levels) and are NULL elsewhere; the brackets are NULL on the grid.
struct LoglikCall {
    const double *X = nullptr;
    int64_t S = 0;
    int32_t C = 0;
    const double *lengths_nm = nullptr;              // host, like n_obs
    double time_ns = 0.0;
    int32_t L = 0;
    int64_t T = 0;
    int32_t plT = 1, tol_exp = 0, max_iter = 0;
    const double *dN = nullptr, *obs = nullptr, *wts = nullptr;
    const int32_t *obs_hi = nullptr;
    const double *obs_dx = nullptr, *obs_h = nullptr;
    int64_t obs_ld = 0;
    const int64_t *n_obs = nullptr;
    const double *sse_cut = nullptr;                 // host: the threshold of the cut entry points
    const double *cut_level = nullptr;               // [C][S]: a level per system (trpl_loglik_cut_levels[_dev]) in the place of sse_cut
    // trpl_loglik_cut_budget[_dev]: budget [S], a level per sample for its total, spent over launches of curves_per_launch curves;
    // cut_level is then the call's OUTPUT (the entry points take it as double *): loglik_dev fills its rows before each launch
    const double *budget = nullptr;
    int32_t curves_per_launch = 0;
    double *P = nullptr, *sse = nullptr, *esum = nullptr;
    int32_t *cut_col = nullptr, *status = nullptr;
    int64_t *iters_total = nullptr;
    int32_t *floor_col = nullptr;
    uint32_t flags = 0;
};
// every check of a trpl_loglik*_dev call, then its launches and the reduction over the curves on `stream` (trpl_api.hip)
int loglik_dev(const LoglikCall &k, hipStream_t stream);

int no_weighted_flag(uint32_t flags);      // TRPL_ERR_ARG when TRPL_FLAG_WEIGHTED reaches an entry point that takes no weights
int no_moments_flag(uint32_t flags);       // TRPL_ERR_ARG when TRPL_FLAG_MOMENTS reaches an entry point without an esum output
int check_grid(int32_t L, int64_t T, int32_t plT, int32_t max_iter, double time_ns);
int check_batch(const LoglikCall &k);       // check_grid, then S >= 0 and C in [1, TRPL_MAX_CURVES]: what every fused-likelihood head shares
// the three bracket arrays of an off-grid call: all or none, and on every time step
int check_interp(const void *obs_hi, const void *obs_dx, const void *obs_h, int32_t plT);
// the observation brackets of trpl_loglik_obs are host data in the host-buffer calls: sorted, in [1, T]
int check_brackets(const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int32_t C, int64_t obs_ld,
                   const int64_t *n_obs, int64_t T);
// time steps a likelihood launch takes: up to the last observation (on-grid), T off-grid
int64_t loglik_steps(bool interp, int32_t C, const int64_t *n_obs, int32_t plT, int64_t T);
// trpl_loglik_multi[_dev], S samples cut into shards: refuses contradictory TRPL_FLAG_KERNEL_* bits, bundles and an n_obs out
// of range, then sets in `flags` the kernel variant a launch of the WHOLE batch runs (TRPL_FLAG_KERNEL_PAIR / _SINGLE), whatever
// the shard sizes: a sample's bits then do not depend on how the batch is cut (the two FAST kernels agree to rounding only)
int pin_sharded_batch(uint32_t &flags, int64_t S, int32_t C, int32_t L, int64_t T, int32_t plT, bool interp, const int64_t *n_obs, int64_t obs_ld);

}  // namespace trpl
