// RANSAC similarity alignment of two reconstructions: b ~ s R a + t from 3-D / 3-D pairs, some of them wrong.
// The pass is the shared one (sfmmin::ransac_pass): the three-item solver of sfm_similarity.h in the shared fit kernel, the
// shared scoring and mask kernels over similarity_model, the selection of sfm_select_best with a sample of three.  Behind it
// the masked closed-form least-squares fit and the refinement of a winner on its inliers, which share the solve of the fit.
//
// Data item i of batch entry b: pairs[b, i] = {ax, ay, az, bx, by, bz}.  Model: 13 doubles R (row-major) | t | s.
//
// The masked fit reduces in two passes — centroid first, then centred moments — over `blocks_for(n)` blocks per entry, each
// leaving one partial record; every consumer adds the partial records in block order, so the sums have one fixed order, no
// floating-point atomics, and a call is bit-reproducible.  The grid depends on n alone.  The bodies of the reduction and
// refinement kernels are the device routines of sfm_similarity_reduce.h, one block's share of one entry each, which the ragged
// call over many sub-model pairs (sfm_align_models.hip) wraps as well.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"
#include "sfm_minimal_score.h"
#include "sfm_similarity.h"
#include "sfm_similarity_reduce.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmsim::blocks_for;
using sfmsim::fold_partials;
using sfmsim::kMoments;
using sfmsim::kScores;
using sfmsim::kSimilarityModel;
using sfmsim::kSimilaritySample;
using sfmsim::kSums;
using sfmsim::model_of;
using sfmsim::RefineState;
using sfmsim::similarity_model;
using sfmsim::similarity_solver;
using sfmsim::SimPair;

static_assert(sizeof(sfm_similarity_refine_info) == 24, "sfm_similarity_refine_info layout is part of the ABI");

constexpr int kBlock = sfmsim::kReduceBlock;

// ---- pass 1: sum a, sum b and the count of the set, one partial record per block; grid (blocks, batch) -------------------
__global__ __launch_bounds__(kBlock) void similarity_sums_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                  const uint8_t* __restrict__ mask, const RefineState* __restrict__ gate,
                                                                  double* __restrict__ part1) {
    const int64_t b = blockIdx.y;
    sfmsim::sums_block(pairs + b * n, n, (int)gridDim.x, (int)blockIdx.x, mask != nullptr ? mask + b * n : nullptr,
                       gate != nullptr ? gate + b : nullptr, part1 + b * gridDim.x * kSums);
}

// ---- pass 2: the centred moments about the centroid of pass 1, one partial record per block; grid (blocks, batch) --------
__global__ __launch_bounds__(kBlock) void similarity_moments_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                     const uint8_t* __restrict__ mask, const RefineState* __restrict__ gate,
                                                                     const double* __restrict__ part1, double* __restrict__ part2) {
    const int64_t b = blockIdx.y;
    sfmsim::moments_block(pairs + b * n, n, (int)gridDim.x, (int)blockIdx.x, mask != nullptr ? mask + b * n : nullptr,
                          gate != nullptr ? gate + b : nullptr, part1 + b * gridDim.x * kSums, part2 + b * gridDim.x * kMoments);
}

// ---- the model of each entry from its partial records; grid (batch), one wave -----------------------------------------
__global__ __launch_bounds__(kWave) void similarity_solve_kernel(const double* __restrict__ part1, const double* __restrict__ part2,
                                                                  int blocks, double* __restrict__ model_out,
                                                                  int32_t* __restrict__ flags_out) {
    __shared__ double sums[kSums];
    __shared__ double moments[kMoments];
    const int64_t b = blockIdx.x;
    fold_partials<kSums>(part1 + b * blocks * kSums, blocks, sums);
    fold_partials<kMoments>(part2 + b * blocks * kMoments, blocks, moments);
    double m[kSimilarityModel];
    const int flag = model_of(sums, moments, m);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSimilarityModel; ++k) model_out[b * kSimilarityModel + k] = m[k];
        flags_out[b] = flag;
    }
}

// ---- refinement: the start; grid (blocks, batch) -----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void similarity_refine_begin_kernel(int64_t n, const double* __restrict__ model_in,
                                                                          const uint8_t* __restrict__ mask_in,
                                                                          const double* __restrict__ err_in, double* __restrict__ model_out,
                                                                          uint8_t* __restrict__ mask_out, double* __restrict__ part0,
                                                                          RefineState* __restrict__ state) {
    const int64_t b = blockIdx.y;
    sfmsim::refine_begin_block(n, (int)gridDim.x, (int)blockIdx.x, model_in + b * kSimilarityModel, mask_in + b * n, err_in + b,
                               model_out + b * kSimilarityModel, mask_out + b * n, part0 + b * gridDim.x, state + b);
}

// ---- refinement: the model of the current inliers and the re-score of every item under it; grid (blocks, batch) ------------
__global__ __launch_bounds__(kBlock) void similarity_refine_score_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                          const RefineState* __restrict__ gate,
                                                                          const double* __restrict__ part1, const double* __restrict__ part2,
                                                                          double thr, double* __restrict__ trial,
                                                                          int32_t* __restrict__ trial_flag, double* __restrict__ part3) {
    const int64_t b = blockIdx.y;
    sfmsim::refine_score_block(pairs + b * n, n, (int)gridDim.x, (int)blockIdx.x, gate + b, part1 + b * gridDim.x * kSums,
                               part2 + b * gridDim.x * kMoments, thr, trial + b * kSimilarityModel, trial_flag + b,
                               part3 + b * gridDim.x * kScores);
}

// ---- refinement: the accept rule, the mask of a kept round, the model and the state; grid (blocks, batch) -------------------
__global__ __launch_bounds__(kBlock) void similarity_refine_accept_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                           const RefineState* __restrict__ state_in,
                                                                           RefineState* __restrict__ state_out,
                                                                           const double* __restrict__ part1, const double* __restrict__ part3,
                                                                           const double* __restrict__ trial,
                                                                           const int32_t* __restrict__ trial_flag, double thr, int aggregation,
                                                                           double* __restrict__ model_out, uint8_t* __restrict__ mask_out) {
    const int64_t b = blockIdx.y;
    sfmsim::refine_accept_block(pairs + b * n, n, (int)gridDim.x, (int)blockIdx.x, state_in + b, state_out + b,
                                part1 + b * gridDim.x * kSums, part3 + b * gridDim.x * kScores, trial + b * kSimilarityModel,
                                trial_flag + b, thr, aggregation, model_out + b * kSimilarityModel, mask_out + b * n);
}

// ---- refinement: the record of each entry; grid (batch), one wave ----------------------------------------------------
__global__ __launch_bounds__(kWave) void similarity_refine_end_kernel(const RefineState* __restrict__ state, const double* __restrict__ part0,
                                                                       int blocks, sfm_similarity_refine_info* __restrict__ info) {
    const int64_t b = blockIdx.x;
    sfmsim::refine_end_entry(state + b, part0 + b * blocks, blocks, info + b);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The pieces of a workspace: those of the masked fit first, so that the fit's workspace is a prefix of the refinement's.
struct Workspace {
    double *part1, *part2, *part0, *part3, *trial;
    int32_t* trial_flag;
    RefineState* state;   // [2, batch]
    int64_t bytes;
};

Workspace carve(void* base, int64_t n, int64_t batch, bool refine) {
    sfmhost::Carver c{(uintptr_t)base, 0};
    const int64_t records = batch * blocks_for(n);
    Workspace w{};
    w.part1 = c.take<double>(records * kSums);
    w.part2 = c.take<double>(records * kMoments);
    if (refine) {
        w.part0 = c.take<double>(records);
        w.part3 = c.take<double>(records * kScores);
        w.trial = c.take<double>(batch * kSimilarityModel);
        w.trial_flag = c.take<int32_t>(batch);
        w.state = c.take<RefineState>(2 * batch);
    }
    w.bytes = c.at;
    return w;
}

bool sizes_ok(int64_t n, int64_t batch) { return n >= kSimilaritySample && n <= 0x7FFFFFFF && batch >= 0 && batch <= 65535; }

int check_reduction_call(const char* fn, int64_t n, int64_t batch) {
    if (n < 0 || batch < 0) return fail_in(fn, "negative size");
    if (!sizes_ok(n, batch)) return fail_in(fn, "need 3 <= n < 2^31 items and batch <= 65535");
    return SFM_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the two reduction passes over the set `mask` (null: every item) of every entry that `gate` (null: all) leaves active
int launch_moments(const SimPair* pairs, int64_t n, int64_t batch, const uint8_t* mask, const RefineState* gate, const Workspace& w,
                   hipStream_t st) {
    const dim3 grid((unsigned)blocks_for(n), (unsigned)batch);
    hipLaunchKernelGGL(similarity_sums_kernel, grid, dim3(kBlock), 0, st, pairs, n, mask, gate, w.part1);
    int rc = check_launch("similarity_sums_kernel");
    if (rc != SFM_OK) return rc;
    hipLaunchKernelGGL(similarity_moments_kernel, grid, dim3(kBlock), 0, st, pairs, n, mask, gate, (const double*)w.part1, w.part2);
    return check_launch("similarity_moments_kernel");
}

int check_pass(const char* fn, int64_t n, int64_t h_count, int64_t batch, const void* pairs) {
    const int rc = sfmhost::check_sizes(fn, kSimilaritySample, n, h_count, batch, {sfmmin::kScoreBlock, sfmmin::kMinimalFitBlock});
    if (rc != SFM_OK) return rc;
    if (!aligned16(pairs)) return fail_in(fn, "pairs must be 16-byte aligned");
    return SFM_OK;
}

constexpr auto launch_score = sfmmin::launch_score<kSimilaritySample, similarity_model>;
constexpr auto launch_mask = sfmmin::launch_mask<kSimilaritySample, similarity_model>;

}  // namespace

extern "C" {

int sfm_similarity_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* pairs, int64_t n,
                               int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation, int32_t* S,
                               double* model, int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result,
                               uint8_t* mask, void* stream) {
    const char* fn = "sfm_similarity_ransac_pass";
    hipStream_t st = (hipStream_t)stream;
    const SimPair* items = (const SimPair*)pairs;
    return sfmmin::ransac_pass(
        fn, check_pass(fn, n, h_count, batch, pairs), kSimilaritySample, h_begin, h_count, batch, min_extra, aggregation, pairs,
        {S, model, flags, cnt, s1, s2, result, mask}, stream,
        [&] {
            return sfmmin::launch_minimal_fit<similarity_solver>(items, use_philox != 0, seed, seed_stride, h_begin, n, h_count, batch, S,
                                                                 model, flags, st);
        },
        [&] { return launch_score(items, n, model, S, h_count, batch, thr, cnt, s1, s2, st); },
        [&] { return launch_mask(items, n, model, S, h_count, batch, result, thr, mask, st); });
}

int64_t sfm_similarity_fit_workspace_bytes(int64_t n, int64_t batch) {
    return sizes_ok(n, batch) ? carve(nullptr, n, batch, false).bytes : -1;
}

int64_t sfm_similarity_refine_workspace_bytes(int64_t n, int64_t batch) {
    return sizes_ok(n, batch) ? carve(nullptr, n, batch, true).bytes : -1;
}

int sfm_similarity_fit_masked(const double* pairs, int64_t n, int64_t batch, const uint8_t* mask, double* model_out, int32_t* flags_out,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "sfm_similarity_fit_masked";
    const int rc = check_reduction_call(fn, n, batch);
    if (rc != SFM_OK) return rc;
    if (batch == 0) return SFM_OK;
    if (!pairs || !model_out || !flags_out || !workspace) return fail_in(fn, "null pointer");
    if (!aligned16(pairs) || !aligned16(workspace)) return fail_in(fn, "pairs and workspace must be 16-byte aligned");
    const Workspace w = carve(workspace, n, batch, false);
    if (workspace_bytes < w.bytes) return fail_in(fn, "workspace too small (sfm_similarity_fit_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const int launched = launch_moments((const SimPair*)pairs, n, batch, mask, nullptr, w, st);
    if (launched != SFM_OK) return launched;
    hipLaunchKernelGGL(similarity_solve_kernel, dim3((unsigned)batch), dim3(kWave), 0, st, (const double*)w.part1, (const double*)w.part2,
                       blocks_for(n), model_out, flags_out);
    return check_launch("similarity_solve_kernel");
}

int sfm_similarity_refine(const double* pairs, int64_t n, int64_t batch, const double* model_in, const uint8_t* mask_in,
                          const double* err_in, double thr, int aggregation, int rounds, double* model_out, uint8_t* mask_out,
                          sfm_similarity_refine_info* info, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "sfm_similarity_refine";
    // every check before the first launch: a refused call has enqueued nothing
    if (rounds < 0) return fail_in(fn, "negative size");
    const int rc = check_reduction_call(fn, n, batch);
    if (rc != SFM_OK) return rc;
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail_in(fn, "unknown aggregation");
    if (batch == 0) return SFM_OK;
    if (!pairs || !model_in || !mask_in || !err_in || !model_out || !mask_out || !info || !workspace) return fail_in(fn, "null pointer");
    if (mask_in == mask_out) return fail_in(fn, "mask_out must not alias mask_in");
    if (!aligned16(pairs) || !aligned16(workspace)) return fail_in(fn, "pairs and workspace must be 16-byte aligned");
    const Workspace w = carve(workspace, n, batch, true);
    if (workspace_bytes < w.bytes) return fail_in(fn, "workspace too small (sfm_similarity_refine_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const SimPair* items = (const SimPair*)pairs;
    const int blocks = blocks_for(n);
    const dim3 grid((unsigned)blocks, (unsigned)batch);
    hipLaunchKernelGGL(similarity_refine_begin_kernel, grid, dim3(kBlock), 0, st, n, model_in, mask_in, err_in, model_out, mask_out, w.part0,
                       w.state);
    int launched = check_launch("similarity_refine_begin_kernel");
    for (int round = 0; round < rounds && launched == SFM_OK; ++round) {
        const RefineState* now = w.state + (round & 1) * batch;
        RefineState* next = w.state + ((round + 1) & 1) * batch;
        launched = launch_moments(items, n, batch, mask_out, now, w, st);
        if (launched != SFM_OK) break;
        hipLaunchKernelGGL(similarity_refine_score_kernel, grid, dim3(kBlock), 0, st, items, n, now, (const double*)w.part1,
                           (const double*)w.part2, thr, w.trial, w.trial_flag, w.part3);
        launched = check_launch("similarity_refine_score_kernel");
        if (launched != SFM_OK) break;
        hipLaunchKernelGGL(similarity_refine_accept_kernel, grid, dim3(kBlock), 0, st, items, n, now, next, (const double*)w.part1,
                           (const double*)w.part3, (const double*)w.trial, (const int32_t*)w.trial_flag, thr, aggregation, model_out,
                           mask_out);
        launched = check_launch("similarity_refine_accept_kernel");
    }
    if (launched != SFM_OK) return launched;
    hipLaunchKernelGGL(similarity_refine_end_kernel, dim3((unsigned)batch), dim3(kWave), 0, st,
                       (const RefineState*)(w.state + (rounds & 1) * batch), (const double*)w.part0, blocks, info);
    return check_launch("similarity_refine_end_kernel");
}

}  // extern "C"
