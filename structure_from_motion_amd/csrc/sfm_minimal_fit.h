// What the minimal solvers of RANSAC share (the six-point DLT and P3P of sfm_pnp.hip, the five-point solver of
// sfm_five_point.hip): the fit kernel, its launcher, the size checks of their entry points and the sequence of a whole pass.
//
// A solver is a struct with
//   kSample, kModel   items per sample (the leading entries of a row of S) and doubles per model;
//   kName             what a failed launch is reported as;
//   Data              what its fit reads besides the sample, passed to the kernel by value;
//   fit(data, b, n, idx, out)   device function: the model of batch entry b from sample idx into out, returns the fit flag;
//   from(data, first)  device function, needed by the ragged fit (sfm_ragged_pass.h) only: the Data whose entry 0 begins at item
//                      `first` of data's, whatever else data holds kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "sfm_common.h"
#include "sfm_math.h"

namespace sfmhost {

inline int fail_in(const char* fn, const char* what) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", fn, what);
    return fail(SFM_EINVAL, msg);
}

// The checks of an entry point that depend on its sizes alone: none negative, sample <= n < 2^31, batch within grid y, and a
// grid over the hypotheses for each block size in `blocks` (one hypothesis per thread).
inline int check_sizes(const char* fn, int sample, int64_t n, int64_t h_count, int64_t batch, std::initializer_list<int> blocks) {
    if (n < 0 || h_count < 0 || batch < 0) return fail_in(fn, "negative size");
    if (n < sample || n > 0x7FFFFFFF) {
        char what[80];
        snprintf(what, sizeof what, "need %d <= n < 2^31 items", sample);
        return fail_in(fn, what);
    }
    bool fits = batch <= 65535;
    for (const int block : blocks) fits = fits && grid_fits(h_count, block, block, batch);
    if (!fits) return fail_in(fn, "size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y)");
    return SFM_OK;
}

// The prologue of an entry point that makes one launch: the outcome of its size checks, nothing to do, a null pointer, the launch.
template <class Launch>
int checked_entry(const char* fn, int sizes, bool nothing, bool null, Launch launch) {
    if (sizes != SFM_OK) return sizes;
    if (nothing) return SFM_OK;
    if (null) return fail_in(fn, "null pointer");
    return launch();
}

}  // namespace sfmhost

namespace sfmmin {

constexpr int kMinimalFitBlock = 64;

// One hypothesis per lane.  Its sample is the first kSample entries of its row of S, or (PHILOX) of
// philox_sample8(seed + b * seed_stride, h_begin + h) — the sampler of sfm_sample_philox — and S then receives all eight, with
// -1 at the positions past the sample that are >= n (so n = kSample is valid, and the host reads the order of the inliers
// from a row without knowing n).
template <class Solver, bool PHILOX>
__global__ __launch_bounds__(kMinimalFitBlock) void minimal_fit_kernel(typename Solver::Data data, uint64_t seed, uint64_t seed_stride,
                                                                       int64_t h_begin, int64_t n, int64_t h_count,
                                                                       int32_t* __restrict__ S, double* __restrict__ model,
                                                                       int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= h_count) return;
    const int64_t b = blockIdx.y;
    const int64_t bh = b * h_count + h;
    int32_t idx[8];
    if constexpr (PHILOX) {
        sfm::philox_sample8(seed + (uint64_t)b * seed_stride, (uint64_t)(h_begin + h), (uint32_t)n, idx);
#pragma unroll
        for (int i = Solver::kSample; i < 8; ++i) idx[i] = i < n ? idx[i] : -1;
#pragma unroll
        for (int i = 0; i < 8; ++i) S[bh * 8 + i] = idx[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) idx[i] = i < Solver::kSample ? S[bh * 8 + i] : 0;
    }
    double out[Solver::kModel];
    const int flag = Solver::fit(data, b, n, idx, out);
#pragma unroll
    for (int i = 0; i < Solver::kModel; ++i) model[bh * Solver::kModel + i] = out[i];
    flags[bh] = flag;
}

// The fit of every hypothesis of `batch` entries; the caller has checked the sizes (check_sizes with kMinimalFitBlock).
template <class Solver>
int launch_minimal_fit(const typename Solver::Data& data, bool philox, uint64_t seed, uint64_t seed_stride, int64_t h_begin, int64_t n,
                       int64_t h_count, int64_t batch, int32_t* S, double* model, int32_t* flags, hipStream_t st) {
    const auto kernel = philox ? minimal_fit_kernel<Solver, true> : minimal_fit_kernel<Solver, false>;
    hipLaunchKernelGGL(kernel, dim3(sfmhost::grid_for(h_count, kMinimalFitBlock), (unsigned)batch), dim3(kMinimalFitBlock), 0, st, data,
                       seed, seed_stride, h_begin, n, h_count, S, model, flags);
    return sfmhost::check_launch(Solver::kName);
}

// The buffers a pass fills, as the C ABI passes them: `mask` may be null (no mask), the others not.
struct PassBuffers {
    int32_t* S;
    double* model;
    int32_t* flags;
    int32_t* cnt;
    double* s1;
    double* s2;
    sfm_select_result* result;
    uint8_t* mask;
};

// One whole pass.  Every argument and grid is checked before the first launch, all that sfm_select_best checks included, so a
// refused call has enqueued nothing: `sizes` is the outcome of the solver's own checks (check_sizes and whatever else its
// launches need), `items` its input pointer.  Then fit() and score() when there are hypotheses, the selection, and mask()
// unless the mask is null.
template <class Fit, class Score, class Mask>
int ransac_pass(const char* fn, int sizes, int sample, int64_t h_begin, int64_t h_count, int64_t batch, double min_extra, int aggregation,
                const void* items, const PassBuffers& o, void* stream, Fit fit, Score score, Mask mask) {
    if (sizes != SFM_OK) return sizes;
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return sfmhost::fail_in(fn, "unknown aggregation");
    if (h_begin < 0) return sfmhost::fail_in(fn, "negative h_begin");
    if (batch == 0) return SFM_OK;
    if (!items || !o.S || !o.model || !o.flags || !o.cnt || !o.s1 || !o.s2 || !o.result) return sfmhost::fail_in(fn, "null pointer");
    int rc = SFM_OK;
    if (h_count > 0 && ((rc = fit()) != SFM_OK || (rc = score()) != SFM_OK)) return rc;
    rc = sfm_select_best(o.cnt, o.s1, o.s2, o.flags, h_count, batch, min_extra, aggregation, 0, sample, o.result, stream);
    if (rc != SFM_OK || o.mask == nullptr) return rc;
    return mask();
}

}  // namespace sfmmin
