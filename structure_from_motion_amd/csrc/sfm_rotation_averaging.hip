// Rotation averaging over a view graph (the NumPy definition, operation by operation, is
// tests/rotation_averaging_oracle.py): one absolute rotation per camera that agrees with the relative rotations of all
// edges at once, by iteratively reweighted Gauss-Newton on the weighted graph Laplacian, each step solved by conjugate
// gradients with the Jacobi preconditioner.  fp64 throughout; off unless asked for.
//
// The parts it shares with translation averaging (the state, the levels, registration, adjacency, the system, the CG
// kernels, the stop decision and the host loop) are csrc/sfm_graph_cg.h; the kernels named graphcg:: below are defined there.
// Set-up, once per call:
//   rotavg_init_kernel       the state, the order's counters, levels, the start rotations, which edges are active
//   graphcg::self_kernel         thread per edge: a self-pair sets the bad flag
//   sfmorder::launch_point_order   the 2Q half-edges (2q -> i_q, 2q + 1 -> j_q) grouped by camera, in increasing
//                            half-edge index inside a camera: the "observations" are the half-edges, the "points" the cameras
//   graphcg::level_kernel      round k, thread per camera: level k (and the tree rotation) from the cameras of level < k
//   graphcg::register_kernel   thread per camera / edge: registered, NaN for an unregistered camera, which edges are used
//   graphcg::adjacency_kernel  thread per half-edge position: the camera at the other end of a used edge, -1 otherwise
//   graphcg::start_kernel      one thread: the status of a call without steps
// Then per step, every launch reading the state first and returning at once after a stop:
//   rotavg_edge_kernel<false>  thread per edge: r = log(R_j^T (R_q R_i)), omega = w rho'(|r|^2), the cost per block
//   graphcg::system_kernel     thread per camera: d_c = sum omega, b_c = sum s omega r over its half-edges in order
//   graphcg::cg_init_kernel    one workgroup: the cost, x = 0, r = b, z = r / d, p = z
//   per CG iteration, each over at most kCgBlocks blocks that leave one partial sum each:
//                            graphcg::cg_apply_kernel     (q_c = sum omega (p_c - p_other) in half-edge order, p . q)
//                            graphcg::cg_update_kernel    (alpha, x, r, z = r / d, r.z and r.r)
//                            graphcg::cg_direction_kernel (rho, beta, p and the stop of CG)
//   rotavg_step_kernel       thread per camera: R_c <- R_c exp([x_c]x), the largest |x_c|_inf
//   graphcg::decide_kernel     one thread: the counters, CONVERGED / MAX_STEPS / CG_FAILED
// and at the end rotavg_edge_kernel<true> (the residuals and the final cost) and rotavg_finish_kernel (info, the filler).
// The host reads three flags (stop, CG done, the last level round that set something) from pinned memory once per batch of
// kRoundBatch level rounds, once per step and once per chunk of kCgChunk CG iterations, and enqueues no more work after a
// stop.  The device state alone decides the result.  No floating-point atomics and no memset nodes: every floating-point sum
// runs in an order fixed by the edge list alone, so a call is bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_graph_cg.h"
#include "sfm_loss.h"
#include "sfm_math.h"
#include "sfm_obs_order.h"
#include "sfm_pnp.h"
#include "sfm_so3.h"

namespace {

using graphcg::is_free;
using graphcg::kOneGroup;
using graphcg::kThreads;
using graphcg::State;
using graphcg::Ws;
using sfm::block_sum;

static_assert(sizeof(sfm_rotavg_info) == 40, "sfm_rotavg_info layout is part of the ABI");
static_assert(sizeof(sfm_rotavg_options) == 40, "sfm_rotavg_options layout is part of the ABI");

static_assert(SFM_ROTAVG_CONVERGED == graphcg::kConverged && SFM_ROTAVG_MAX_STEPS == graphcg::kMaxSteps &&
                  SFM_ROTAVG_CG_FAILED == graphcg::kCgFailed && SFM_ROTAVG_BAD_INDEX == graphcg::kBadIndex,
              "the shared kernels write these statuses");
static_assert(SFM_ROTAVG_INIT_TREE == graphcg::kInitTree && SFM_ROTAVG_INIT_GIVEN == graphcg::kInitGiven,
              "graphcg::check_entry tests these");

// The bytes of the workspace, carved from `base` (0: the size only); -1 for sizes the call refuses
int64_t carve(uintptr_t base, int64_t C, int64_t Q, Ws* w) {
    if (!graphcg::sizes_ok(C, Q)) return -1;
    sfmhost::Carver k{base, 0};
    graphcg::carve(k, C, Q, w);
    return k.at;
}

struct Args {
    int C, Q, root;
    bool given;
    const int32_t* pairs;
    const double *rel, *weights, *initial;
    double* R;
    uint8_t* registered;
    int32_t* level;   // the caller's copy of the levels, or nullptr
    double* residual;
    SFM_DEVICE void clear_camera(int64_t c) const {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[9 * c + k] = (double)NAN;
    }
};

// Thread i: the state (thread 0), the order's counters of camera i, its level and start rotation, and whether edge i is active
__global__ __launch_bounds__(kThreads) void rotavg_init_kernel(Args a, Ws w) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) *w.st = State{};
    if (i <= a.C) w.po.off[i] = 0;
    if (i < a.C) {
        w.level[i] = i == a.root ? 0 : -1;
        double* R = a.R + 9 * i;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            R[k] = a.given ? a.initial[9 * i + k] : (i == a.root ? (k % 4 == 0 ? 1.0 : 0.0) : (double)NAN);
    }
    if (i < a.Q) {
        const double wq = a.weights[i];
        bool ok = isfinite(wq) && wq > 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) ok = ok && isfinite(a.rel[9 * i + k]);
        w.used[i] = ok ? 1 : 0;
    }
}

// out = A B, out = A^T B (row-major 3 x 3), every entry (a0 b0 + a1 b1) + a2 b2
SFM_DEVICE void mul(const double* A, const double* B, double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

SFM_DEVICE void mul_t(const double* A, const double* B, double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}

// The tree start: camera c takes its rotation through half-edge `best`
struct Tree {
    static constexpr bool kOn = true;
    static SFM_DEVICE void place(const Args& a, int c, int best) {
        const int q = best >> 1;
        const double* Ro = a.R + 9 * (int64_t)a.pairs[best ^ 1];
        double Rq[9], Rc[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Rq[e] = a.rel[9 * (int64_t)q + e];
        if (best & 1) mul(Rq, Ro, Rc);   // c is the j end: R_c = R_q R_i
        else mul_t(Rq, Ro, Rc);          // c is the i end: R_c = R_q^T R_j
#pragma unroll
        for (int e = 0; e < 9; ++e) a.R[9 * (int64_t)c + e] = Rc[e];
    }
};

// Thread per edge: r = log(R_j^T (R_q R_i)), e = |r|^2, omega = w rho'(e), w rho(e) summed per block.  kFinal (after the
// steps): the residual |r| instead of r and omega, NaN for an edge that is not used; runs after a stop too.
template <bool kFinal>
__global__ __launch_bounds__(kThreads) void rotavg_edge_kernel(Args a, sfmloss::Loss loss, Ws w) {
    __shared__ double part[kThreads / kWave];
    __shared__ double total[1];
    if (kFinal ? w.st->bad : w.st->stop) return;
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double cost[1] = {0.0};
    if (q < a.Q) {
        if (w.used[q] == 2) {
            double Rq[9], A[9], D[9], r[3];
#pragma unroll
            for (int e = 0; e < 9; ++e) Rq[e] = a.rel[9 * q + e];
            mul(Rq, a.R + 9 * (int64_t)a.pairs[2 * q], A);
            mul_t(a.R + 9 * (int64_t)a.pairs[2 * q + 1], A, D);
            sfmso3::log_map(D, r);
            const double e = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            const double wq = a.weights[q];
            cost[0] = wq * sfmloss::rho(loss, e);
            if (kFinal) {
                a.residual[q] = sqrt(e);
            } else {
                w.omega[q] = wq * sfmloss::weight(loss, e);
#pragma unroll
                for (int k = 0; k < 3; ++k) w.rvec[3 * q + k] = r[k];
            }
        } else if (kFinal) {
            a.residual[q] = (double)NAN;
        }
    }
    block_sum<1, kThreads>(cost, part, total);
    if (threadIdx.x == 0) w.cost_part[blockIdx.x] = total[0];
}

// Thread per free camera: R_c <- R_c exp([x_c]x) = exp([R_c x_c]x) R_c by the Rodrigues update of csrc/sfm_pnp.h, and the
// largest |x_c|_inf (an integer maximum over the bits of non-negative doubles).  Nothing after a failed CG.
__global__ __launch_bounds__(kThreads) void rotavg_step_kernel(Args a, Ws w) {
    if (w.st->stop || w.st->cg_fail) return;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= a.C || !is_free(a, w, c)) return;
    const double x[3] = {w.x[3 * (int64_t)c], w.x[3 * (int64_t)c + 1], w.x[3 * (int64_t)c + 2]};
    double pose[12], delta[6], out[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) pose[k] = a.R[9 * (int64_t)c + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pose[9 + k] = 0.0;
        delta[3 + k] = 0.0;
        delta[k] = (pose[3 * k] * x[0] + pose[3 * k + 1] * x[1]) + pose[3 * k + 2] * x[2];
    }
    sfmpnp::apply_step(pose, delta, out);
#pragma unroll
    for (int k = 0; k < 9; ++k) a.R[9 * (int64_t)c + k] = out[k];
    graphcg::record_step(w, x);
}

// One workgroup, after the final edge pass: after a bad index the filler of the rotations and residuals; graphcg::finish_info
// has the rest of the filler and info.
__global__ __launch_bounds__(kOneGroup) void rotavg_finish_kernel(Args a, int blocks, Ws w, sfm_rotavg_info* __restrict__ info) {
    if (w.st->bad) {
        for (int64_t i = threadIdx.x; i < 9 * (int64_t)a.C; i += kOneGroup) a.R[i] = (double)NAN;
        for (int64_t i = threadIdx.x; i < a.Q; i += kOneGroup) a.residual[i] = (double)NAN;
    }
    graphcg::finish_info(a, blocks, w, info);
}

// The launches that are rotation averaging's own (graphcg::run has the rest)
struct Driver {
    const Args& a;
    const sfmloss::Loss& loss;
    const Ws& w;
    sfm_rotavg_info* info;
    hipStream_t st;
    void init(unsigned grid) { hipLaunchKernelGGL(rotavg_init_kernel, dim3(grid), dim3(kThreads), 0, st, a, w); }
    bool tree_given() const { return a.given; }
    void edge(int, unsigned grid) { hipLaunchKernelGGL(rotavg_edge_kernel<false>, dim3(grid), dim3(kThreads), 0, st, a, loss, w); }
    void step(unsigned grid) { hipLaunchKernelGGL(rotavg_step_kernel, dim3(grid), dim3(kThreads), 0, st, a, w); }
    void finish(unsigned grid, int qblocks) {
        hipLaunchKernelGGL(rotavg_edge_kernel<true>, dim3(grid), dim3(kThreads), 0, st, a, loss, w);
        hipLaunchKernelGGL(rotavg_finish_kernel, dim3(1), dim3(kOneGroup), 0, st, a, qblocks, w, info);
    }
};

}  // namespace

extern "C" {

int64_t sfm_average_rotations_workspace_bytes(int64_t cameras, int64_t edges) {
    Ws w;
    return carve(0, cameras, edges, &w);
}

int sfm_average_rotations(int64_t cameras, int64_t edges, const int32_t* pairs, const double* relative,
                          const double* weights, int64_t root, const double* initial, const sfm_rotavg_options* options,
                          double* rotations, uint8_t* registered, int32_t* level, double* residual, sfm_rotavg_info* info,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    const sfm_rotavg_options o = options ? *options : sfm_rotavg_options{};
    const bool given = o.init == SFM_ROTAVG_INIT_GIVEN;
    const bool pointers = rotations && registered && info && workspace && (!given || initial) &&
                          (edges == 0 || (pairs && relative && weights && residual));
    Ws w;
    int32_t* flags;
    const int rc = graphcg::check_entry("sfm_average_rotations", "ROTAVG", cameras, edges, root, options != nullptr, o, nullptr,
                                        pointers, workspace, workspace_bytes, carve((uintptr_t)workspace, cameras, edges, &w),
                                        &flags);
    if (rc != SFM_OK) return rc;
    const sfmloss::Loss loss{o.loss, 0, o.loss_scale, o.loss_scale * o.loss_scale};
    const Args a{(int)cameras, (int)edges, (int)root, given, pairs, relative, weights, initial, rotations, registered, level, residual};
    const graphcg::Limits limits{o.max_steps, o.max_cg_iterations, 0, o.cg_tolerance, o.step_tolerance};
    Driver drv{a, loss, w, info, (hipStream_t)stream};
    return graphcg::run<Tree>(a, limits, w, drv, flags, (hipStream_t)stream, "sfm_average_rotations");
}

}  // extern "C"
