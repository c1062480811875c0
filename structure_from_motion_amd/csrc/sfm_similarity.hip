// RANSAC similarity alignment of two reconstructions: b ~ s R a + t from 3-D / 3-D pairs, some of them wrong.
// The pass is the shared one (sfmmin::ransac_pass): the three-item solver of sfm_similarity.h in the shared fit kernel, the
// shared scoring and mask kernels over similarity_model, the selection of sfm_select_best with a sample of three.  Behind it
// the masked closed-form least-squares fit and the refinement of a winner on its inliers, which share the solve of the fit.
//
// Data item i of batch entry b: pairs[b, i] = {ax, ay, az, bx, by, bz}.  Model: 13 doubles R (row-major) | t | s.
//
// The masked fit reduces in two passes — centroid first, then centred moments — over `blocks_for(n)` blocks per entry, each
// leaving one partial record; every consumer adds the partial records in block order, so the sums have one fixed order, no
// floating-point atomics, and a call is bit-reproducible.  The grid depends on n alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"
#include "sfm_minimal_score.h"
#include "sfm_similarity.h"

namespace {

using sfm::block_sum;
using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmsim::kSimilarityModel;
using sfmsim::kSimilaritySample;
using sfmsim::Moments;
using sfmsim::similarity_model;
using sfmsim::similarity_solver;
using sfmsim::SimPair;

static_assert(sizeof(sfm_similarity_refine_info) == 24, "sfm_similarity_refine_info layout is part of the ABI");

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kItemsPerBlock = 2048;   // below this an entry's reduction is one block
constexpr int kMaxBlocks = 128;        // partial records per entry at most
constexpr int kSums = 7;               // sum a (3) | sum b (3) | count
constexpr int kMoments = 11;           // M (9) | sa2 | sb2
constexpr int kScores = 3;             // count | sum e | sum e^2

// What a refinement carries from round to round, per entry; double-buffered, so that the blocks of a launch read one copy
// while block 0 writes the other.
struct RefineState {
    double err;       // aggregated error of the model kept so far
    double cnt;       // its inlier count; < 0: not counted yet (no round has run)
    int32_t active;   // 0 once a round stopped early or was rejected
    int32_t accepted, rounds_run, pad;
};
static_assert(sizeof(RefineState) == 32, "two doubles and four words");

// The sum over an entry's `blocks` partial records of K doubles, in block order, into total (LDS, K doubles): valid for every
// thread after the call.
template <int K>
SFM_DEVICE void fold_partials(const double* __restrict__ partial, int blocks, double* total) {
    if (threadIdx.x < K) {
        double acc = partial[threadIdx.x];
        for (int j = 1; j < blocks; ++j) acc += partial[(int64_t)j * K + threadIdx.x];
        total[threadIdx.x] = acc;
    }
    __syncthreads();
}

// The means of the set from the folded sums: mu = sum / count.
SFM_DEVICE void centroids(const double* sums, double (&mua)[3], double (&mub)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mua[k] = sums[k] / sums[6];
        mub[k] = sums[3 + k] / sums[6];
    }
}

// The model of the set whose folded sums and moments are given (LDS): sfmsim::solve, the solve of the minimal fit.
SFM_DEVICE int model_of(const double* sums, const double* moments, double (&out)[kSimilarityModel]) {
    Moments mo;
    centroids(sums, mo.mua, mo.mub);
#pragma unroll
    for (int k = 0; k < 9; ++k) mo.M[k] = moments[k];
    mo.sa2 = moments[9];
    mo.sb2 = moments[10];
    return sfmsim::solve(mo, out);
}

// ---- pass 1: sum a, sum b and the count of the set, one partial record per block; grid (blocks, batch) -------------------
__global__ __launch_bounds__(kBlock) void similarity_sums_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                  const uint8_t* __restrict__ mask, const RefineState* __restrict__ gate,
                                                                  double* __restrict__ part1) {
    __shared__ double part[kWaves * kSums];
    __shared__ double total[kSums];
    const int64_t b = blockIdx.y;
    if (gate != nullptr && !gate[b].active) return;   // block-uniform
    const SimPair* __restrict__ P = pairs + b * n;
    const uint8_t* __restrict__ m = mask != nullptr ? mask + b * n : nullptr;
    double v[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (m != nullptr && m[i] == 0) continue;
        const SimPair q = P[i];
        v[0] += q.ax; v[1] += q.ay; v[2] += q.az;
        v[3] += q.bx; v[4] += q.by; v[5] += q.bz;
        v[6] += 1.0;
    }
    block_sum<kSums, kBlock>(v, part, total);
    if (threadIdx.x < kSums) part1[(b * gridDim.x + blockIdx.x) * kSums + threadIdx.x] = total[threadIdx.x];
}

// ---- pass 2: the centred moments about the centroid of pass 1, one partial record per block; grid (blocks, batch) --------
__global__ __launch_bounds__(kBlock) void similarity_moments_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                     const uint8_t* __restrict__ mask, const RefineState* __restrict__ gate,
                                                                     const double* __restrict__ part1, double* __restrict__ part2) {
    __shared__ double part[kWaves * kMoments];
    __shared__ double total[kMoments];
    __shared__ double sums[kSums];
    const int64_t b = blockIdx.y;
    if (gate != nullptr && !gate[b].active) return;   // block-uniform
    fold_partials<kSums>(part1 + b * gridDim.x * kSums, (int)gridDim.x, sums);
    double mua[3], mub[3];
    centroids(sums, mua, mub);
    const SimPair* __restrict__ P = pairs + b * n;
    const uint8_t* __restrict__ m = mask != nullptr ? mask + b * n : nullptr;
    double v[kMoments];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) v[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (m != nullptr && m[i] == 0) continue;
        const SimPair q = P[i];
        const double da[3] = {q.ax - mua[0], q.ay - mua[1], q.az - mua[2]};
        const double db[3] = {q.bx - mub[0], q.by - mub[1], q.bz - mub[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) v[3 * r + k] += db[r] * da[k];
        v[9] += (da[0] * da[0] + da[1] * da[1]) + da[2] * da[2];
        v[10] += (db[0] * db[0] + db[1] * db[1]) + db[2] * db[2];
    }
    block_sum<kMoments, kBlock>(v, part, total);
    if (threadIdx.x < kMoments) part2[(b * gridDim.x + blockIdx.x) * kMoments + threadIdx.x] = total[threadIdx.x];
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
// mask_out = (mask_in != 0), its count per block into part0; block 0 copies the model and opens the state.
__global__ __launch_bounds__(kBlock) void similarity_refine_begin_kernel(int64_t n, const double* __restrict__ model_in,
                                                                          const uint8_t* __restrict__ mask_in,
                                                                          const double* __restrict__ err_in, double* __restrict__ model_out,
                                                                          uint8_t* __restrict__ mask_out, double* __restrict__ part0,
                                                                          RefineState* __restrict__ state) {
    __shared__ double part[kWaves];
    __shared__ double total[1];
    const int64_t b = blockIdx.y;
    double v[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint8_t m = mask_in[b * n + i] != 0 ? 1 : 0;
        mask_out[b * n + i] = m;
        v[0] += (double)m;
    }
    block_sum<1, kBlock>(v, part, total);
    if (threadIdx.x == 0) part0[b * gridDim.x + blockIdx.x] = total[0];
    if (blockIdx.x == 0) {
        if (threadIdx.x < kSimilarityModel) model_out[b * kSimilarityModel + threadIdx.x] = model_in[b * kSimilarityModel + threadIdx.x];
        if (threadIdx.x == 0) state[b] = RefineState{err_in[b], -1.0, 1, 0, 0, 0};
    }
}

// ---- refinement: the model of the current inliers (every block solves it; block 0 leaves it in `trial`) and the re-score of
// every item under it, one partial record per block; grid (blocks, batch) ---------------------------------------------------
__global__ __launch_bounds__(kBlock) void similarity_refine_score_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                          const RefineState* __restrict__ gate,
                                                                          const double* __restrict__ part1, const double* __restrict__ part2,
                                                                          double thr, double* __restrict__ trial,
                                                                          int32_t* __restrict__ trial_flag, double* __restrict__ part3) {
    __shared__ double part[kWaves * kScores];
    __shared__ double total[kScores];
    __shared__ double sums[kSums];
    __shared__ double moments[kMoments];
    const int64_t b = blockIdx.y;
    if (!gate[b].active) return;   // block-uniform
    fold_partials<kSums>(part1 + b * gridDim.x * kSums, (int)gridDim.x, sums);
    fold_partials<kMoments>(part2 + b * gridDim.x * kMoments, (int)gridDim.x, moments);
    double m[kSimilarityModel];
    const int flag = model_of(sums, moments, m);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSimilarityModel; ++k) trial[b * kSimilarityModel + k] = m[k];
        trial_flag[b] = flag;
    }
    if (!(sums[6] >= (double)kSimilaritySample) || flag != 0) return;   // block-uniform: the round stops in the accept kernel
    const SimPair* __restrict__ P = pairs + b * n;
    double c[kScores] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double e = sfmsim::pair_error(m, P[i]);
        if (e <= thr) {
            c[0] += 1.0;
            c[1] += e;
            c[2] += e * e;
        }
    }
    block_sum<kScores, kBlock>(c, part, total);
    if (threadIdx.x < kScores) part3[(b * gridDim.x + blockIdx.x) * kScores + threadIdx.x] = total[threadIdx.x];
}

// ---- refinement: the accept rule (sfmfit::refit_wins), decided alike by every block from the same records;
// a kept round rewrites the mask, and block 0 moves the model and the state on; grid (blocks, batch) -----------------------
__global__ __launch_bounds__(kBlock) void similarity_refine_accept_kernel(const SimPair* __restrict__ pairs, int64_t n,
                                                                           const RefineState* __restrict__ state_in,
                                                                           RefineState* __restrict__ state_out,
                                                                           const double* __restrict__ part1, const double* __restrict__ part3,
                                                                           const double* __restrict__ trial,
                                                                           const int32_t* __restrict__ trial_flag, double thr, int aggregation,
                                                                           double* __restrict__ model_out, uint8_t* __restrict__ mask_out) {
    __shared__ double sums[kSums];
    __shared__ double scores[kScores];
    const int64_t b = blockIdx.y;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    const RefineState st = state_in[b];
    if (!st.active) {   // block-uniform
        if (writer) state_out[b] = st;
        return;
    }
    fold_partials<kSums>(part1 + b * gridDim.x * kSums, (int)gridDim.x, sums);
    const double current = sums[6];
    const bool enough = current >= (double)kSimilaritySample;
    if (!enough || trial_flag[b] != 0) {   // block-uniform: fewer than three inliers, or a degenerate set
        if (writer) state_out[b] = RefineState{st.err, current, 0, st.accepted, st.rounds_run + (enough ? 1 : 0), 0};
        return;
    }
    fold_partials<kScores>(part3 + b * gridDim.x * kScores, (int)gridDim.x, scores);
    const double cnt = scores[0];
    const double err = sfmfit::aggregate_error(aggregation, (int)cnt, scores[1], scores[2], 0);
    if (!sfmfit::refit_wins(cnt, err, current, st.err)) {   // block-uniform
        if (writer) state_out[b] = RefineState{st.err, current, 0, st.accepted, st.rounds_run + 1, 0};
        return;
    }
    double m[kSimilarityModel];
#pragma unroll
    for (int k = 0; k < kSimilarityModel; ++k) m[k] = trial[b * kSimilarityModel + k];
    const SimPair* __restrict__ P = pairs + b * n;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        mask_out[b * n + i] = sfmsim::pair_error(m, P[i]) <= thr ? 1 : 0;
    if (blockIdx.x == 0 && threadIdx.x < kSimilarityModel) model_out[b * kSimilarityModel + threadIdx.x] = m[threadIdx.x];
    if (writer) state_out[b] = RefineState{err, cnt, 1, st.accepted + 1, st.rounds_run + 1, 0};
}

// ---- refinement: the record of each entry; grid (batch), one wave ----------------------------------------------------
__global__ __launch_bounds__(kWave) void similarity_refine_end_kernel(const RefineState* __restrict__ state, const double* __restrict__ part0,
                                                                       int blocks, sfm_similarity_refine_info* __restrict__ info) {
    __shared__ double counted[1];
    const int64_t b = blockIdx.x;
    fold_partials<1>(part0 + b * blocks, blocks, counted);
    if (threadIdx.x == 0) {
        const RefineState st = state[b];
        sfm_similarity_refine_info r;
        r.error = st.err;
        r.count = (int32_t)(st.cnt < 0.0 ? counted[0] : st.cnt);
        r.accepted = st.accepted;
        r.rounds_run = st.rounds_run;
        r.reserved = 0;
        info[b] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int blocks_for(int64_t n) {
    const int64_t g = (n + kItemsPerBlock - 1) / kItemsPerBlock;
    return (int)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}

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
