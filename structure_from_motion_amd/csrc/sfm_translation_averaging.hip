// Translation averaging over a view graph (the NumPy definition, operation by operation, is
// tests/translation_averaging_oracle.py): one position per camera from one unit world direction per edge,
// v_q ~ c_j - c_i, by the bilinear angle-based objective of Zhuang, Cheong and Lee (BATA, CVPR 2018):
// minimise sum w rho(|d_q (c_j - c_i) - v_q|^2) over the positions and the scales d_q >= 0, alternating the closed-form
// scales with an iteratively reweighted step on the weighted graph Laplacian.  fp64 throughout; off unless asked for.
//
// The levels, the registration, the adjacency, the system, the conjugate gradients, the stop decision and the host loop are
// csrc/sfm_graph_cg.h, shared with rotation averaging.  This file's own launches:
//   transavg_init_kernel          thread i: the state, the order's counter and the start of camera i, the world direction of edge
//                                 i (copied, or -(R_j^T t) / |t| from the global rotations) and whether it is active
//   TreeStart (in the level rounds)  c_child = c_parent + v at the j end, c_parent - v at the i end
//   transavg_edge_kernel<warm, final>  thread per edge: the scale d, r = v - d Delta, e = |r|^2, omega = w rho'(e); it stores
//                                 omega d^2 and r / d, so that the shared system is the one of the step; the cost per block.
//                                 final: the angle between Delta and v and the scale instead
//   transavg_step_kernel          thread per free camera: c <- c + x, the largest |x_c|_inf
//   transavg_finish_kernel        one workgroup: info; after a bad index the filler of every output
// No floating-point atomics and no memset nodes: a call is reproducible bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_graph_cg.h"
#include "sfm_loss.h"
#include "sfm_math.h"

namespace {

using graphcg::is_free;
using graphcg::kOneGroup;
using graphcg::kThreads;
using graphcg::State;
using graphcg::Ws;
using sfm::block_sum;

static_assert(sizeof(sfm_transavg_info) == 40, "sfm_transavg_info layout is part of the ABI");
static_assert(sizeof(sfm_transavg_options) == 48, "sfm_transavg_options layout is part of the ABI");
static_assert(SFM_TRANSAVG_CONVERGED == graphcg::kConverged && SFM_TRANSAVG_MAX_STEPS == graphcg::kMaxSteps &&
                  SFM_TRANSAVG_CG_FAILED == graphcg::kCgFailed && SFM_TRANSAVG_BAD_INDEX == graphcg::kBadIndex,
              "the shared kernels write these statuses");
static_assert(SFM_TRANSAVG_INIT_TREE == graphcg::kInitTree && SFM_TRANSAVG_INIT_GIVEN == graphcg::kInitGiven,
              "graphcg::check_entry tests these");

struct Args {
    int C, Q, root;
    bool given;
    const int32_t* pairs;
    const double *dir, *rot;   // [3Q] v or t; [9C] the global rotations or nullptr (dir is v)
    const double *weights, *initial;
    double* c;                 // [3C] the positions
    uint8_t* registered;
    int32_t* level;            // the caller's copy of the levels, or nullptr
    double *residual, *scale;  // [Q] each
    double* v;                 // [3Q] workspace: the world directions
    SFM_DEVICE void clear_camera(int64_t i) const {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[3 * i + k] = (double)NAN;
    }
};

// The bytes of the workspace, carved from `base` (0: the size only); -1 for sizes the call refuses
int64_t carve(uintptr_t base, int64_t C, int64_t Q, Ws* w, double** v) {
    if (!graphcg::sizes_ok(C, Q)) return -1;
    sfmhost::Carver k{base, 0};
    graphcg::carve(k, C, Q, w);
    *v = k.take<double>(3 * Q);
    return k.at;
}

// Thread i: the state (thread 0), the order's counter of camera i, its level and start position; the world direction of edge i
// and whether it is active.  With rotations v = -(u / n), u_k = (R_j[0][k] t0 + R_j[1][k] t1) + R_j[2][k] t2,
// n = sqrt((t0 t0 + t1 t1) + t2 t2); an index j outside the cameras is not followed.
__global__ __launch_bounds__(kThreads) void transavg_init_kernel(Args a, Ws w) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) *w.st = State{};
    if (i <= a.C) w.po.off[i] = 0;
    if (i < a.C) {
        w.level[i] = i == a.root ? 0 : -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.c[3 * i + k] = a.given ? a.initial[3 * i + k] : (i == a.root ? 0.0 : (double)NAN);
    }
    if (i < a.Q) {
        const double wq = a.weights[i];
        bool ok = isfinite(wq) && wq > 0.0;
        const double t[3] = {a.dir[3 * i], a.dir[3 * i + 1], a.dir[3 * i + 2]};
        double v[3] = {t[0], t[1], t[2]};
        if (a.rot) {
            const int j = a.pairs[2 * i + 1];
            if (j < 0 || j >= a.C) {
                ok = false;   // the point order, which runs next, raises the bad flag for this index
            } else {
                const double* R = a.rot + 9 * (int64_t)j;
                const double n = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
                ok = ok && n > 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) ok = ok && isfinite(R[k]);
#pragma unroll
                for (int k = 0; k < 3; ++k) v[k] = -(((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]) / n);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ok = ok && isfinite(v[k]);
            a.v[3 * i + k] = v[k];
        }
        w.used[i] = ok ? 1 : 0;
    }
}

// The tree start: camera c through half-edge `best`: c_other + v at the j end, c_other - v at the i end
struct TreeStart {
    static constexpr bool kOn = true;
    static SFM_DEVICE void place(const Args& a, int c, int best) {
        const double* co = a.c + 3 * (int64_t)a.pairs[best ^ 1];
        const double* v = a.v + 3 * (int64_t)(best >> 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) a.c[3 * (int64_t)c + k] = (best & 1) ? co[k] + v[k] : co[k] - v[k];
    }
};

// Thread per used edge: Delta = c_j - c_i, n2 = (D0 D0 + D1 D1) + D2 D2, dv = (D0 v0 + D1 v1) + D2 v2, the scale
// d = max(dv, 0) / n2 (0 when n2 = 0; kWarm: 1), r = v - d Delta, e = (r0 r0 + r1 r1) + r2 r2, omega = w rho'(e); stored are
// omega (d d) and r / d (0 when d = 0); w rho(e) summed per block.  kFinal (after the steps, never kWarm; runs after a stop
// too): the angle atan2(|Delta x v|, dv) and d instead, NaN for an edge that is not used.
template <bool kWarm, bool kFinal>
__global__ __launch_bounds__(kThreads) void transavg_edge_kernel(Args a, sfmloss::Loss loss, Ws w) {
    __shared__ double part[kThreads / kWave];
    __shared__ double total[1];
    if (kFinal ? w.st->bad : w.st->stop) return;
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double cost[1] = {0.0};
    if (q < a.Q) {
        if (w.used[q] == 2) {
            const double* ci = a.c + 3 * (int64_t)a.pairs[2 * q];
            const double* cj = a.c + 3 * (int64_t)a.pairs[2 * q + 1];
            const double v[3] = {a.v[3 * q], a.v[3 * q + 1], a.v[3 * q + 2]};
            const double D[3] = {cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]};
            const double n2 = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2];
            const double dv = (D[0] * v[0] + D[1] * v[1]) + D[2] * v[2];
            const double d = kWarm ? 1.0 : (n2 == 0.0 ? 0.0 : fmax(dv, 0.0) / n2);
            const double r[3] = {v[0] - d * D[0], v[1] - d * D[1], v[2] - d * D[2]};
            const double e = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            const double wq = a.weights[q];
            cost[0] = wq * sfmloss::rho(loss, e);
            if (kFinal) {
                const double x[3] = {D[1] * v[2] - D[2] * v[1], D[2] * v[0] - D[0] * v[2], D[0] * v[1] - D[1] * v[0]};
                a.residual[q] = atan2(sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), dv);
                a.scale[q] = d;
            } else {
                w.omega[q] = (wq * sfmloss::weight(loss, e)) * (d * d);
#pragma unroll
                for (int k = 0; k < 3; ++k) w.rvec[3 * q + k] = d == 0.0 ? 0.0 : r[k] / d;
            }
        } else if (kFinal) {
            a.residual[q] = (double)NAN;
            a.scale[q] = (double)NAN;
        }
    }
    block_sum<1, kThreads>(cost, part, total);
    if (threadIdx.x == 0) w.cost_part[blockIdx.x] = total[0];
}

// Thread per free camera: c <- c + x, and the largest |x_c|_inf.  Nothing after a failed CG.
__global__ __launch_bounds__(kThreads) void transavg_step_kernel(Args a, Ws w) {
    if (w.st->stop || w.st->cg_fail) return;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= a.C || !is_free(a, w, c)) return;
    const double x[3] = {w.x[3 * (int64_t)c], w.x[3 * (int64_t)c + 1], w.x[3 * (int64_t)c + 2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) a.c[3 * (int64_t)c + k] = a.c[3 * (int64_t)c + k] + x[k];
    graphcg::record_step(w, x);
}

// One workgroup, after the final edge pass: after a bad index the filler of the positions, residuals and scales;
// graphcg::finish_info has the rest of the filler and info.
__global__ __launch_bounds__(kOneGroup) void transavg_finish_kernel(Args a, int blocks, Ws w, sfm_transavg_info* __restrict__ info) {
    if (w.st->bad) {
        for (int64_t i = threadIdx.x; i < 3 * (int64_t)a.C; i += kOneGroup) a.c[i] = (double)NAN;
        for (int64_t i = threadIdx.x; i < a.Q; i += kOneGroup) {
            a.residual[i] = (double)NAN;
            a.scale[i] = (double)NAN;
        }
    }
    graphcg::finish_info(a, blocks, w, info);
}

// The launches that are translation averaging's own (graphcg::run has the rest)
struct Driver {
    const Args& a;
    const sfmloss::Loss& loss;
    const Ws& w;
    int warmup_steps;
    sfm_transavg_info* info;
    hipStream_t st;
    void init(unsigned grid) { hipLaunchKernelGGL(transavg_init_kernel, dim3(grid), dim3(kThreads), 0, st, a, w); }
    bool tree_given() const { return a.given; }
    void edge(int step, unsigned grid) {
        if (step < warmup_steps)
            hipLaunchKernelGGL((transavg_edge_kernel<true, false>), dim3(grid), dim3(kThreads), 0, st, a, loss, w);
        else
            hipLaunchKernelGGL((transavg_edge_kernel<false, false>), dim3(grid), dim3(kThreads), 0, st, a, loss, w);
    }
    void step(unsigned grid) { hipLaunchKernelGGL(transavg_step_kernel, dim3(grid), dim3(kThreads), 0, st, a, w); }
    void finish(unsigned grid, int qblocks) {
        hipLaunchKernelGGL((transavg_edge_kernel<false, true>), dim3(grid), dim3(kThreads), 0, st, a, loss, w);
        hipLaunchKernelGGL(transavg_finish_kernel, dim3(1), dim3(kOneGroup), 0, st, a, qblocks, w, info);
    }
};

}  // namespace

extern "C" {

int64_t sfm_average_translations_workspace_bytes(int64_t cameras, int64_t edges) {
    Ws w;
    double* v;
    return carve(0, cameras, edges, &w, &v);
}

int sfm_average_translations(int64_t cameras, int64_t edges, const int32_t* pairs, const double* directions,
                             const double* rotations, const double* weights, int64_t root, const double* initial,
                             const sfm_transavg_options* options, double* positions, uint8_t* registered, int32_t* level,
                             double* residual, double* scale, sfm_transavg_info* info, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    const sfm_transavg_options o = options ? *options : sfm_transavg_options{};
    const char* own = o.warmup_steps < 0 ? "warmup_steps must be at least 0" : o.reserved != 0 ? "reserved must be 0" : nullptr;
    const bool given = o.init == SFM_TRANSAVG_INIT_GIVEN;
    const bool pointers = positions && registered && info && workspace && (!given || initial) &&
                          (edges == 0 || (pairs && directions && weights && residual && scale));
    Ws w;
    double* v;
    int32_t* flags;
    const int rc = graphcg::check_entry("sfm_average_translations", "TRANSAVG", cameras, edges, root, options != nullptr, o, own,
                                        pointers, workspace, workspace_bytes,
                                        carve((uintptr_t)workspace, cameras, edges, &w, &v), &flags);
    if (rc != SFM_OK) return rc;
    const sfmloss::Loss loss{o.loss, 0, o.loss_scale, o.loss_scale * o.loss_scale};
    const Args a{(int)cameras, (int)edges, (int)root, given, pairs, directions, rotations, weights, initial, positions, registered,
                 level, residual, scale, v};
    const graphcg::Limits limits{o.max_steps, o.max_cg_iterations, o.warmup_steps, o.cg_tolerance, o.step_tolerance};
    Driver drv{a, loss, w, o.warmup_steps, info, (hipStream_t)stream};
    return graphcg::run<TreeStart>(a, limits, w, drv, flags, (hipStream_t)stream, "sfm_average_translations");
}

}  // extern "C"
