// Bundle adjustment: Levenberg-Marquardt over C <= 64 camera poses and P points on the sum of the PnP scorer's squared
// reprojection errors, with the Schur complement on the points (the NumPy oracle is tests/bundle_oracle.py).
// fp64 throughout; off unless asked for.  The LM loop is csrc/sfm_bundle_lm.h's; this file solves the damped reduced
// camera system S dc = b densely, with W = Jc^T Jp stored per observation.
//
// Set-up, once per call: the free cameras' slots from the mask (on the device: no host round trip), then the point-major
// and the camera-major orders of csrc/sfm_obs_order.h (inside a camera the observations are sorted by point, which the
// merge-joins of the reduced camera system walk).  Then per LM trial step, every launch reading the LM state in the
// workspace first and returning at once after a stop:
//   linearize_kernel<true>  (only after an accepted step)  thread per point: V_p, g_p, and W = Jc^T Jp per observation
//   camera_kernel           (only after an accepted step)  block per free camera: U_c and g_c over its observations
//   point_kernel            thread per point: V_p* = V_p + lambda diag V_p and its inverse
//   bundle_schur_kernel     block per upper block (a, b) of free cameras: sum_p W_ap V_p*^-1 W_bp^T by a merge-join of
//                           the two cameras' point-sorted lists (and the right-hand side term on the diagonal blocks)
//   bundle_solve_kernel     one workgroup: dense Cholesky of S (6F x 6F, in LDS up to kLdsFree free cameras), both
//                           triangular solves, then finish_step: the camera steps and the trial poses
//   bundle_trial_kernel     thread per point: back-substitution dX_p, the trial point, its observations' trial cost
//   decide_kernel<256>      one workgroup: the cost in a fixed order, accept / reject, lambda, the gauge scale, stops
//   commit_kernel           an accepted trial becomes the current estimate (rescaled when one camera is fixed)
// No floating-point atomics anywhere: every sum runs in an order fixed by the sizes alone, so a call is bit-reproducible.
//
// A robust loss (csrc/sfm_loss.h) runs the kRobust = true forms of linearize_kernel, camera_kernel and
// bundle_trial_kernel: W, V, U and both gradients are stored weighted, so the Schur complement, the solve and the
// back-substitution are the same launches, and the workspace is the same size.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_bundle_lm.h"
#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_pnp.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmlm::kThreads;
using sfmlm::Lm;
using sfmlm::Obs;
using sfmlm::State;
using sfmpnp::camera_from;
using sfmpnp::pnp_score;
using sfmpnp::PnPCamera;

constexpr int kMaxCameras = sfmlm::kLdsCameras;
constexpr int kLdsFree = 30;                 // S (packed lower triangle) in LDS up to this many free cameras: 127 KiB
constexpr int kSolveThreads = 1024;          // the one-workgroup solve
constexpr int kMaxSolve = 6 * (kMaxCameras - 1);

static_assert(sizeof(sfm_bundle_info) == 32, "sfm_bundle_info layout is part of the ABI");

struct Ws {
    Lm lm;
    const int32_t* pos_c;   // camera-major position -> point-major position (set after the orders are enqueued)
    double *W, *blk, *rhs, *S;
};

// The workspace from `base` (0: sizes only); its size in bytes.
int64_t carve(uintptr_t base, int64_t C, int64_t P, int64_t M, Ws* w, sfmlm::Core* core) {
    const int64_t F = C > 0 ? C - 1 : 0;   // at most: at least one camera is fixed
    sfmlm::Carver k{base, 0};
    State* st = k.take<State>(1);
    *core = sfmlm::carve_core(k, C, P, M, F, st);
    w->lm = core->lm;
    w->pos_c = nullptr;
    w->W = k.take<double>(18 * M);
    w->blk = k.take<double>(36 * (F * (F + 1) / 2));
    w->rhs = k.take<double>(6 * C);
    w->S = k.take<double>(F > kLdsFree ? (6 * F) * (6 * F + 1) / 2 : 0);
    return k.at;
}

SFM_DEVICE int64_t lower(int i, int j) { return (int64_t)i * (i + 1) / 2 + j; }   // i >= j, packed lower triangle

// The state, and the free cameras' slots from the mask of fixed cameras
__global__ __launch_bounds__(kMaxCameras) void bundle_init_kernel(uint64_t fixed, int C, Lm w) {
    const int c = threadIdx.x;
    if (c == 0) sfmlm::init_state(w.st);
    if (c >= C) return;
    if ((fixed >> c) & 1ull) {
        w.slot[c] = -1;
    } else {
        const int s = c - __popcll(fixed & ((1ull << c) - 1ull));
        w.slot[c] = s;
        w.freec[s] = c;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// The dense solve of the damped reduced camera system.
// ------------------------------------------------------------------------------------------------------------------------
// Block per upper block (a, b), a <= b, of the free cameras' slots: blk = sum over pairs (i in a, j in b) of observations
// of the same moving point p of W_i V_p*^-1 W_j^T.  Thread t takes a contiguous chunk of a's list and walks b's list
// beside it from a binary search.  On the diagonal blocks also rhs_a = sum_i W_i V_p*^-1 g_p.
__global__ __launch_bounds__(kThreads) void bundle_schur_kernel(int F, Ws w) {
    __shared__ double part[kThreads / kWave * 42];
    __shared__ double total[42];
    const Lm& l = w.lm;
    if (l.st->stop || l.st->fail) return;
    // block -> (a, b) in row-major order of the upper triangle
    int a = 0, idx = blockIdx.x;
    while (idx >= F - a) {
        idx -= F - a;
        ++a;
    }
    const int b = a + idx;
    const int ca = l.freec[a], cb = l.freec[b];
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; ++k) acc[k] = 0.0;
    const int alo = l.off_c[ca], na = l.off_c[ca + 1] - alo;
    const int blo = l.off_c[cb], bhi = l.off_c[cb + 1];
    const int chunk = (na + kThreads - 1) / kThreads;
    const int i0 = alo + min(na, (int)threadIdx.x * chunk), i1 = alo + min(na, ((int)threadIdx.x + 1) * chunk);
    if (i0 < i1) {
        int j = blo, hi = bhi;   // first entry of b's list with point >= the chunk's first point
        const int32_t first = l.pt_c[i0];
        while (j < hi) {
            const int mid = (j + hi) >> 1;
            if (l.pt_c[mid] < first) j = mid + 1;
            else hi = mid;
        }
        for (int i = i0; i < i1; ++i) {
            const int32_t p = l.pt_c[i];
            if (l.off_p[p + 1] - l.off_p[p] < 2) continue;
            while (j < bhi && l.pt_c[j] < p) ++j;
            if (j >= bhi) break;
            if (l.pt_c[j] != p) continue;
            double Vi[3][3];
            sfmlm::sym3(l.Vi + 6 * (int64_t)p, Vi);
            const double* Wi = w.W + 18 * (int64_t)w.pos_c[i];
            double Y[6][3];
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y) Y[x][y] = (Wi[3 * x] * Vi[0][y] + Wi[3 * x + 1] * Vi[1][y]) + Wi[3 * x + 2] * Vi[2][y];
            for (int k = j; k < bhi && l.pt_c[k] == p; ++k) {
                const double* Wj = w.W + 18 * (int64_t)w.pos_c[k];
#pragma unroll
                for (int x = 0; x < 6; ++x)
#pragma unroll
                    for (int y = 0; y < 6; ++y) acc[6 * x + y] += (Y[x][0] * Wj[3 * y] + Y[x][1] * Wj[3 * y + 1]) + Y[x][2] * Wj[3 * y + 2];
            }
            if (a == b) {
                const double* g = l.gp + 3 * (int64_t)p;
#pragma unroll
                for (int x = 0; x < 6; ++x) acc[36 + x] += (Y[x][0] * g[0] + Y[x][1] * g[1]) + Y[x][2] * g[2];
            }
        }
    }
    sfm::block_sum<42, kThreads>(acc, part, total);
    if (threadIdx.x < 36) w.blk[36 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
    else if (a == b && threadIdx.x < 42) w.rhs[6 * a + threadIdx.x - 36] = total[threadIdx.x];
}

// One workgroup: S = U* - blk (lower triangle, packed), right-hand side -g_c + rhs, Cholesky, both triangular solves;
// then the camera steps and the trial poses (finish_step).  S lives in LDS (kLds) or in the workspace.
template <bool kLds>
__global__ __launch_bounds__(kSolveThreads) void bundle_solve_kernel(int F, int C, const double* __restrict__ poses, Ws w) {
    constexpr int kLdsN = 6 * kLdsFree;
    __shared__ double lds[kLds ? kLdsN * (kLdsN + 1) / 2 : 1];
    __shared__ double y[kMaxSolve];
    __shared__ int ok;
    State* st = w.lm.st;
    if (st->stop) return;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int kWaves = kSolveThreads / kWave;
    if (tid == 0) st->need_lin = 0;   // the linearisation kernels of this step have run
    const int n = 6 * F;
    double* A = kLds ? lds : w.S;
    if (tid == 0) ok = !st->fail;
    const double lambda = st->lambda;
    __syncthreads();
    if (ok) {
        for (int64_t e = tid; e < (int64_t)n * (n + 1) / 2; e += kSolveThreads) {
            // packed lower index e -> (i, j), i >= j
            int i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
            while ((int64_t)i * (i + 1) / 2 > e) --i;
            while ((int64_t)(i + 1) * (i + 2) / 2 <= e) ++i;
            const int j = (int)(e - (int64_t)i * (i + 1) / 2);
            const int a = j / 6, b = i / 6, r = j % 6, s = i % 6;   // a <= b: element (6a + r, 6b + s) of the upper blocks
            const int64_t pair = (int64_t)a * F - (int64_t)a * (a - 1) / 2 + (b - a);
            double v = -w.blk[36 * pair + 6 * r + s];
            if (a == b) {
                const double u = w.lm.U[21 * w.lm.freec[a] + sfmlm::upper6(r, s)];
                v += r == s ? u + lambda * u : u;
            }
            A[e] = v;
        }
        for (int i = tid; i < n; i += kSolveThreads) y[i] = -w.lm.gc[6 * w.lm.freec[i / 6] + i % 6] + w.rhs[i];
    }
    __syncthreads();
    // right-looking Cholesky, column by column
    // tid 0 writes `ok` only between the first barrier of an iteration and the one before it: every thread reads it after
    for (int j = 0; j < n; ++j) {
        if (tid == 0) {
            const double d = A[lower(j, j)];
            if (!(d > 0.0) || !isfinite(d)) ok = 0;
            else A[lower(j, j)] = sqrt(d);
        }
        __syncthreads();
        if (!ok) break;
        const double piv = A[lower(j, j)];
        for (int i = j + 1 + tid; i < n; i += kSolveThreads) A[lower(i, j)] /= piv;
        __syncthreads();
        for (int i = j + 1 + wave; i < n; i += kWaves) {
            const double lij = A[lower(i, j)];
            for (int k = j + 1 + lane; k <= i; k += kWave) A[lower(i, k)] -= lij * A[lower(k, j)];
        }
        __syncthreads();
    }
    if (ok) {
        for (int j = 0; j < n; ++j) {   // L z = y
            if (tid == 0) y[j] /= A[lower(j, j)];
            __syncthreads();
            const double yj = y[j];
            for (int i = j + 1 + tid; i < n; i += kSolveThreads) y[i] -= A[lower(i, j)] * yj;
            __syncthreads();
        }
        for (int j = n - 1; j >= 0; --j) {   // L^T x = z
            if (tid == 0) {
                y[j] /= A[lower(j, j)];
                if (!isfinite(y[j])) ok = 0;
            }
            __syncthreads();
            const double xj = y[j];
            for (int i = tid; i < j; i += kSolveThreads) y[i] -= A[lower(j, i)] * xj;
            __syncthreads();
        }
    }
    sfmlm::finish_step<kSolveThreads>(ok, y, C, poses, w.lm);
}

// Thread per point: dX_p = V_p*^-1 (-g_p - sum over its free-camera observations of W^T dc), the trial point, the trial cost
// of its observations (kRobust: the sum of rho) and its share of |delta|^2 and |x|^2; partials per block.
template <bool kRobust>
__global__ __launch_bounds__(kThreads) void bundle_trial_kernel(Obs obs, int P, PnPCamera cam, const double* __restrict__ points,
                                                                int C, Ws w) {
    __shared__ double pose[kMaxCameras * 12];
    __shared__ double dc[kMaxCameras * 6];
    __shared__ double part[kThreads / kWave * 3];
    __shared__ double total[3];
    const Lm& l = w.lm;
    if (l.st->stop || !l.st->step_ok) return;
    for (int k = threadIdx.x; k < 12 * C; k += kThreads) pose[k] = l.tpose[k];
    for (int k = threadIdx.x; k < 6 * C; k += kThreads) dc[k] = l.dc[k];
    __syncthreads();
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};   // cost | |dX|^2 | |X|^2
    if (p < P) {
        double X[3] = {points[3 * (int64_t)p], points[3 * (int64_t)p + 1], points[3 * (int64_t)p + 2]};
        const int q0 = l.off_p[p], q1 = l.off_p[p + 1];
        if (q1 - q0 >= 2) {
            double t[3] = {-l.gp[3 * (int64_t)p], -l.gp[3 * (int64_t)p + 1], -l.gp[3 * (int64_t)p + 2]};
            for (int q = q0; q < q1; ++q) {
                const int c = l.camp[q];
                if (l.slot[c] < 0) continue;
                const double* Wq = w.W + 18 * (int64_t)q;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < 6; ++i) s += Wq[3 * i + j] * dc[6 * c + i];
                    t[j] -= s;
                }
            }
            double Vi[3][3];
            sfmlm::sym3(l.Vi + 6 * (int64_t)p, Vi);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double d = (Vi[i][0] * t[0] + Vi[i][1] * t[1]) + Vi[i][2] * t[2];
                a[1] += d * d;
                a[2] += X[i] * X[i];
                X[i] += d;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) l.tpts[3 * (int64_t)p + i] = X[i];
        for (int q = q0; q < q1; ++q) {
            const int m = l.ord_p[q];
            const double e = pnp_score(pose + 12 * l.camp[q], cam, X[0], X[1], X[2], obs.uv[2 * (int64_t)m], obs.uv[2 * (int64_t)m + 1]);
            a[0] += kRobust ? sfmloss::rho(l.loss, e) : e;
        }
    }
    sfm::block_sum<3, kThreads>(a, part, total);
    if (threadIdx.x < 3) l.part[3 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

__global__ void bundle_finish_kernel(Lm w, sfm_bundle_info* __restrict__ info) { sfmlm::write_info(w.st, info); }

// A checked call: everything enqueue needs.
struct Job {
    PnPCamera cam;
    int64_t C, P, M;
    uint64_t mask;
    const double *poses_in, *points_in;
    Obs obs;
    int max_steps;
    double *poses_out, *points_out;
    sfm_bundle_info* info;
    hipStream_t st;
};

// Enqueue the whole call; kRobust picks the kernels of a non-squared loss (w.lm.loss).
template <bool kRobust>
int enqueue(const Job& job, Ws& w, const sfmlm::Core& core) {
    const PnPCamera& cam = job.cam;
    const int64_t C = job.C, P = job.P, M = job.M;
    const uint64_t mask = job.mask;
    const double *poses_in = job.poses_in, *points_in = job.points_in;
    double *poses_out = job.poses_out, *points_out = job.points_out;
    const int max_steps = job.max_steps;
    hipStream_t st = job.st;
    const Obs& obs = job.obs;
    const int F = (int)C - __builtin_popcountll(mask);
    const int f = __builtin_ctzll(mask);                                        // the gauge's fixed camera
    const int anchor = C - F == 1 && F > 0 ? __builtin_ctzll(~mask) : -1;       // one fixed camera: the lowest free one
    const unsigned pgrid = sfmhost::grid_for(P, kThreads), icgrid = sfmhost::grid_for(P > C ? P : C, kThreads);
    const int pblocks = (int)((P + kThreads - 1) / kThreads);
    const unsigned pairs = (unsigned)(F * (F + 1) / 2);

    // the output starts as the input; the state and the point counters start at zero
    if (poses_out != poses_in && hipMemcpyAsync(poses_out, poses_in, 8 * 12 * C, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return check_launch("sfm_bundle_adjust: copy poses");
    if (P > 0 && points_out != points_in &&
        hipMemcpyAsync(points_out, points_in, 8 * 3 * P, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return check_launch("sfm_bundle_adjust: copy points");
    if (hipMemsetAsync(w.lm.off_p, 0, 4 * (P + 1), st) != hipSuccess) return check_launch("sfm_bundle_adjust: clear the counters");
    hipLaunchKernelGGL(bundle_init_kernel, dim3(1), dim3(kMaxCameras), 0, st, mask, (int)C, w.lm);
    w.pos_c = sfmlm::launch_orders(obs, M, C, P, core, st);
    auto linearize = [&]() {
        hipLaunchKernelGGL((sfmlm::linearize_kernel<true, kRobust>), dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, poses_out,
                           points_out, (int)C, w.lm, w.W);
        if (F > 0)
            hipLaunchKernelGGL(sfmlm::camera_kernel<kRobust>, dim3((unsigned)F), dim3(kThreads), 0, st, obs, cam, poses_out, points_out,
                               w.lm);
    };
    linearize();
    hipLaunchKernelGGL(sfmlm::start_kernel<kThreads>, dim3(1), dim3(kThreads), 0, st, pblocks, f, anchor, max_steps, poses_out,
                       w.lm);
    for (int step = 0; step < max_steps; ++step) {
        linearize();
        hipLaunchKernelGGL(sfmlm::point_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, w.lm);
        if (pairs > 0) hipLaunchKernelGGL(bundle_schur_kernel, dim3(pairs), dim3(kThreads), 0, st, F, w);
        if (F <= kLdsFree)
            hipLaunchKernelGGL(bundle_solve_kernel<true>, dim3(1), dim3(kSolveThreads), 0, st, F, (int)C, poses_out, w);
        else
            hipLaunchKernelGGL(bundle_solve_kernel<false>, dim3(1), dim3(kSolveThreads), 0, st, F, (int)C, poses_out, w);
        hipLaunchKernelGGL(bundle_trial_kernel<kRobust>, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, points_out, (int)C, w);
        hipLaunchKernelGGL(sfmlm::decide_kernel<kThreads>, dim3(1), dim3(kThreads), 0, st, pblocks, anchor, max_steps, w.lm);
        hipLaunchKernelGGL(sfmlm::commit_kernel, dim3(icgrid), dim3(kThreads), 0, st, (int)P, (int)C, anchor, poses_out,
                           points_out, w.lm);
    }
    hipLaunchKernelGGL(bundle_finish_kernel, dim3(1), dim3(1), 0, st, w.lm, job.info);
    return check_launch("sfm_bundle_adjust");
}

}  // namespace

extern "C" {

int64_t sfm_bundle_workspace_bytes(int64_t cameras, int64_t points, int64_t observations) {
    if (cameras < 1 || cameras > kMaxCameras || points < 0 || observations < 0 || points > 0x7FFFFFFF ||
        observations > 0x7FFFFFFF)
        return -1;
    Ws w;
    sfmlm::Core core;
    return carve(0, cameras, points, observations, &w, &core);
}

int sfm_bundle_adjust_ex(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                         const double* poses_in, const double* points_in, const int32_t* camera_index,
                         const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                         double* points_out, sfm_bundle_info* info, void* workspace, int64_t workspace_bytes, void* stream,
                         const sfm_bundle_options* options) {
    // every check before the first launch: a refused call has enqueued nothing
    if (cameras < 1 || points < 0 || observations < 0 || max_steps < 0) return fail(SFM_EINVAL, "sfm_bundle_adjust: bad size");
    if (cameras > kMaxCameras) return fail(SFM_EINVAL, "sfm_bundle_adjust: more than 64 cameras");
    if (points > 0x7FFFFFFF || observations > 0x7FFFFFFF)
        return fail(SFM_EINVAL, "sfm_bundle_adjust: points and observations must be below 2^31");
    sfmloss::Loss loss;
    if (!sfmloss::from_options(options, loss))
        return fail(SFM_EINVAL, "sfm_bundle_adjust: options need a loss in 0..2, reserved = 0 and a loss_scale > 0 with a normal finite square");
    PnPCamera cam;
    const int rc = camera_from(K, cam, "sfm_bundle_adjust");
    if (rc != SFM_OK) return rc;
    if (!fixed) return fail(SFM_EINVAL, "sfm_bundle_adjust: null pointer (fixed)");
    uint64_t mask = 0;
    for (int64_t c = 0; c < cameras; ++c)
        if (fixed[c]) mask |= 1ull << c;
    if (mask == 0) return fail(SFM_EINVAL, "sfm_bundle_adjust: at least one camera must be fixed");
    if (!poses_in || !poses_out || !info || !workspace || (points > 0 && (!points_in || !points_out)) ||
        (observations > 0 && (!camera_index || !point_index || !pixels)))
        return fail(SFM_EINVAL, "sfm_bundle_adjust: null pointer");
    const int64_t C = cameras, P = points, M = observations;
    Ws w;
    sfmlm::Core core;
    if (workspace_bytes < carve((uintptr_t)workspace, C, P, M, &w, &core))
        return fail(SFM_EINVAL, "sfm_bundle_adjust: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_bundle_adjust: workspace must be 16-byte aligned");

    w.lm.loss = loss;
    const Job job{cam, C, P, M, mask, poses_in, points_in, Obs{camera_index, point_index, pixels}, max_steps, poses_out, points_out,
                  info, (hipStream_t)stream};
    return loss.kind == SFM_BUNDLE_LOSS_SQUARED ? enqueue<false>(job, w, core) : enqueue<true>(job, w, core);
}

int sfm_bundle_adjust(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                      const double* poses_in, const double* points_in, const int32_t* camera_index,
                      const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                      double* points_out, sfm_bundle_info* info, void* workspace, int64_t workspace_bytes, void* stream) {
    return sfm_bundle_adjust_ex(K, cameras, points, observations, fixed, poses_in, points_in, camera_index, point_index, pixels,
                                max_steps, poses_out, points_out, info, workspace, workspace_bytes, stream, nullptr);
}

}  // extern "C"
