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
//
// sfm_bundle_adjust_calibrated runs the kCal = true forms: up to three intrinsics theta = (f, cx, cy) shared by
// all cameras border the reduced system with q = 1..3 rows.  The camera lives in the workspace (sfmlm::Calib: the current one
// and the trial one).  linearize_kernel adds W_qp per point and U_qq, g_q per block, camera_kernel U_cq, the diagonal blocks
// of bundle_schur_kernel sum_i W_i V_p*^-1 W_qp^T, and one more launch per trial step,
//   bundle_border_kernel    thread per point: sum_p W_qp V_p*^-1 W_qp^T and sum_p W_qp V_p*^-1 g_p, partials per block
// before bundle_solve_kernel, which factors the order 6F + q system and sets the trial camera; bundle_trial_kernel
// back-substitutes with -W_qp^T dtheta, commit_kernel keeps the trial camera.  Every intrinsics array is 3 wide, a held
// intrinsic's entries are zero and the solve skips its row.  A call without a free intrinsic is kCal = false: the
// instantiations and the bits of before.
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
                                             // (132 KiB with the border of a calibrating call)
constexpr int kSolveThreads = 1024;          // the one-workgroup solve
constexpr int kMaxSolve = 6 * (kMaxCameras - 1);
constexpr int kBorder = 3;                   // the intrinsics a calibrating call can free

static_assert(sizeof(sfm_bundle_info) == 32, "sfm_bundle_info layout is part of the ABI");

struct Ws {
    Lm lm;
    const int32_t* pos_c;   // camera-major position -> point-major position (set after the orders are enqueued)
    double *W, *blk, *rhs, *S;
    double* Sq;             // kCal: sum_i W_i V_p*^-1 W_qp^T (6 x 3) per free camera's slot
};

// The workspace from `base` (0: sizes only); its size in bytes.
int64_t carve(uintptr_t base, int64_t C, int64_t P, int64_t M, Ws* w, sfmlm::Core* core, bool cal = false) {
    const int64_t F = C > 0 ? C - 1 : 0;   // at most: at least one camera is fixed
    sfmlm::Carver k{base, 0};
    State* st = k.take<State>(1);
    *core = sfmlm::carve_core(k, C, P, M, F, st);
    w->lm = core->lm;
    w->pos_c = nullptr;
    w->W = k.take<double>(18 * M);
    w->blk = k.take<double>(36 * (F * (F + 1) / 2));
    w->rhs = k.take<double>(6 * C);
    const int64_t n = 6 * F + (cal ? kBorder : 0);
    w->S = k.take<double>(F > kLdsFree ? n * (n + 1) / 2 : 0);
    w->Sq = nullptr;
    if (cal) {   // after everything a plain call has
        const int64_t blocks = (P + kThreads - 1) / kThreads;
        w->lm.cal = k.take<sfmlm::Calib>(1);
        w->lm.Wq = k.take<double>(9 * P);
        w->lm.Ucq = k.take<double>(18 * C);
        w->lm.qpart = k.take<double>(18 * (blocks > 0 ? blocks : 1));
        w->Sq = k.take<double>(18 * F);
    }
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
// The free intrinsics of a refine mask: their number, and the index in (f, cx, cy) of the s-th
SFM_DEVICE int border_order(int refine) { return (refine & 1) + (refine & 2); }
SFM_DEVICE int border_index(int refine, int s) { return (refine & 1) ? s : s + 1; }

__global__ void bundle_calib_init_kernel(sfmlm::Calib* cal, PnPCamera cam, int refine) {
    cal->cam = cam;
    cal->trial = cam;
    cal->dq[0] = cal->dq[1] = cal->dq[2] = 0.0;
    cal->refine = refine;
    cal->pad = 0;
}

// Block per upper block (a, b), a <= b, of the free cameras' slots: blk = sum over pairs (i in a, j in b) of observations
// of the same moving point p of W_i V_p*^-1 W_j^T.  Thread t takes a contiguous chunk of a's list and walks b's list
// beside it from a binary search.  On the diagonal blocks also rhs_a = sum_i W_i V_p*^-1 g_p, and (kCal) Sq_a =
// sum_i W_i V_p*^-1 W_qp^T.
template <bool kCal>
__global__ __launch_bounds__(kThreads) void bundle_schur_kernel(int F, Ws w) {
    constexpr int kSums = kCal ? 60 : 42;
    __shared__ double part[kThreads / kWave * kSums];
    __shared__ double total[kSums];
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
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
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
                if (kCal) {
                    const double* Wq = l.Wq + 9 * (int64_t)p;
#pragma unroll
                    for (int x = 0; x < 6; ++x)
#pragma unroll
                        for (int y = 0; y < 3; ++y)
                            acc[42 + 3 * x + y] += (Y[x][0] * Wq[3 * y] + Y[x][1] * Wq[3 * y + 1]) + Y[x][2] * Wq[3 * y + 2];
                }
            }
        }
    }
    sfm::block_sum<kSums, kThreads>(acc, part, total);
    if (threadIdx.x < 36) w.blk[36 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
    else if (a == b && threadIdx.x < 42) w.rhs[6 * a + threadIdx.x - 36] = total[threadIdx.x];
    else if (kCal && a == b && threadIdx.x < 60) w.Sq[18 * a + threadIdx.x - 42] = total[threadIdx.x];
}

// Thread per point: a moving point's share of sum_p W_qp V_p*^-1 W_qp^T (upper 6) and of sum_p W_qp V_p*^-1 g_p; partials
// per block, behind the block's U_qq and g_q.
__global__ __launch_bounds__(kThreads) void bundle_border_kernel(int P, Lm l) {
    __shared__ double part[kThreads / kWave * 9];
    __shared__ double total[9];
    if (l.st->stop || l.st->fail) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < P && l.off_p[p + 1] - l.off_p[p] >= 2) {
        double Vi[3][3];
        sfmlm::sym3(l.Vi + 6 * (int64_t)p, Vi);
        const double* Wq = l.Wq + 9 * (int64_t)p;
        const double* g = l.gp + 3 * (int64_t)p;
        double Y[3][3];
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) Y[x][y] = (Wq[3 * x] * Vi[0][y] + Wq[3 * x + 1] * Vi[1][y]) + Wq[3 * x + 2] * Vi[2][y];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
#pragma unroll
            for (int y = x; y < 3; ++y)
                a[sfmlm::upper3(x, y)] = (Y[x][0] * Wq[3 * y] + Y[x][1] * Wq[3 * y + 1]) + Y[x][2] * Wq[3 * y + 2];
            a[6 + x] = (Y[x][0] * g[0] + Y[x][1] * g[1]) + Y[x][2] * g[2];
        }
    }
    sfm::block_sum<9, kThreads>(a, part, total);
    if (threadIdx.x < 9) l.qpart[18 * (int64_t)blockIdx.x + 9 + threadIdx.x] = total[threadIdx.x];
}

// One workgroup: S = U* - blk (lower triangle, packed), right-hand side -g_c + rhs, Cholesky, both triangular solves;
// then the camera steps and the trial poses (finish_step).  S lives in LDS (kLds) or in the workspace.  kCal: the system
// has the q free intrinsics behind the cameras (S_aq = U_aq - Sq_a, S_qq = U_qq* - sum W_qp V_p*^-1 W_qp^T, right-hand side
// -g_q + sum W_qp V_p*^-1 g_p, the sums over the `blocks` point blocks in their order), and the step sets the trial camera:
// a trial k00 that is not finite, is zero or changes sign rejects the step.
template <bool kLds, bool kCal>
__global__ __launch_bounds__(kSolveThreads) void bundle_solve_kernel(int F, int C, const double* __restrict__ poses, Ws w,
                                                                     int blocks) {
    constexpr int kLdsN = 6 * kLdsFree + (kCal ? kBorder : 0);
    __shared__ double lds[kLds ? kLdsN * (kLdsN + 1) / 2 : 1];
    __shared__ double y[kMaxSolve + (kCal ? kBorder : 0)];
    __shared__ double qsum[kCal ? 18 : 1];   // U_qq (upper 6) | g_q | sum W_qp V_p*^-1 W_qp^T (upper 6) | sum W_qp V_p*^-1 g_p
    __shared__ double dq[kCal ? kBorder : 1];   // the trial step of (f, cx, cy), by thread 0
    __shared__ int ok;
    State* st = w.lm.st;
    if (st->stop) return;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int kWaves = kSolveThreads / kWave;
    if (tid == 0) st->need_lin = 0;   // the linearisation kernels of this step have run
    const int refine = kCal ? w.lm.cal->refine : 0;
    const int n = 6 * F + (kCal ? border_order(refine) : 0);
    double* A = kLds ? lds : w.S;
    if (tid == 0) ok = !st->fail;
    const double lambda = st->lambda;
    if (kCal && tid < 18) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += w.lm.qpart[18 * (int64_t)b + tid];
        qsum[tid] = s;
    }
    __syncthreads();
    if (ok) {
        for (int64_t e = tid; e < (int64_t)n * (n + 1) / 2; e += kSolveThreads) {
            // packed lower index e -> (i, j), i >= j
            int i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
            while ((int64_t)i * (i + 1) / 2 > e) --i;
            while ((int64_t)(i + 1) * (i + 2) / 2 <= e) ++i;
            const int j = (int)(e - (int64_t)i * (i + 1) / 2);
            if (kCal && i >= 6 * F) {   // a row of the border
                const int qi = border_index(refine, i - 6 * F);
                if (j < 6 * F) {
                    const int a = j / 6, r = j % 6;
                    A[e] = w.lm.Ucq[18 * w.lm.freec[a] + 3 * r + qi] - w.Sq[18 * a + 3 * r + qi];
                } else {
                    const int k = sfmlm::upper3(border_index(refine, j - 6 * F), qi);
                    const double u = qsum[k];
                    A[e] = -qsum[9 + k] + (i == j ? u + lambda * u : u);
                }
                continue;
            }
            const int a = j / 6, b = i / 6, r = j % 6, s = i % 6;   // a <= b: element (6a + r, 6b + s) of the upper blocks
            const int64_t pair = (int64_t)a * F - (int64_t)a * (a - 1) / 2 + (b - a);
            double v = -w.blk[36 * pair + 6 * r + s];
            if (a == b) {
                const double u = w.lm.U[21 * w.lm.freec[a] + sfmlm::upper6(r, s)];
                v += r == s ? u + lambda * u : u;
            }
            A[e] = v;
        }
        for (int i = tid; i < 6 * F; i += kSolveThreads) y[i] = -w.lm.gc[6 * w.lm.freec[i / 6] + i % 6] + w.rhs[i];
        if (kCal && tid < n - 6 * F) y[6 * F + tid] = -qsum[6 + border_index(refine, tid)] + qsum[15 + border_index(refine, tid)];
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
    if (kCal) {
        if (tid == 0) {
            sfmlm::Calib* cal = w.lm.cal;
            PnPCamera t = cal->cam;
            dq[0] = dq[1] = dq[2] = 0.0;
            if (ok) {
                for (int s = 0; s < n - 6 * F; ++s) dq[border_index(refine, s)] = y[6 * F + s];
                if (refine & SFM_BUNDLE_REFINE_FOCAL) {
                    const double f = t.k00 + dq[0];
                    if (!isfinite(f) || f == 0.0 || (f < 0.0) != (t.k00 < 0.0)) {
                        ok = 0;
                    } else {
                        const double ratio = f / t.k00;
                        t.k00 = f;
                        t.k01 *= ratio;
                        t.k10 *= ratio;
                        t.k11 *= ratio;
                    }
                }
                t.k02 += dq[1];
                t.k12 += dq[2];
            }
            if (!ok) {
                t = cal->cam;
                dq[0] = dq[1] = dq[2] = 0.0;
            }
            cal->trial = t;
            for (int k = 0; k < 3; ++k) cal->dq[k] = dq[k];
        }
        __syncthreads();
    }
    sfmlm::finish_step<kSolveThreads>(ok, y, C, poses, w.lm);
    if (kCal && tid == 0 && ok) {   // the intrinsics' share of |delta|^2 and |x|^2, behind the cameras'
        const PnPCamera& k = w.lm.cal->cam;
        st->dn_c += (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
        if (refine & SFM_BUNDLE_REFINE_FOCAL) st->xn_c += k.k00 * k.k00;
        if (refine & SFM_BUNDLE_REFINE_PRINCIPAL_POINT) st->xn_c += k.k02 * k.k02 + k.k12 * k.k12;
    }
}

// Thread per point: dX_p = V_p*^-1 (-g_p - sum over its free-camera observations of W^T dc), the trial point, the trial cost
// of its observations (kRobust: the sum of rho) and its share of |delta|^2 and |x|^2; partials per block.  kCal: under the
// trial camera, with -W_qp^T dtheta in the back-substitution.
template <bool kRobust, bool kCal>
__global__ __launch_bounds__(kThreads) void bundle_trial_kernel(Obs obs, int P, PnPCamera cam, const double* __restrict__ points,
                                                                int C, Ws w) {
    __shared__ double pose[kMaxCameras * 12];
    __shared__ double dc[kMaxCameras * 6];
    __shared__ double part[kThreads / kWave * 3];
    __shared__ double total[3];
    const Lm& l = w.lm;
    if (l.st->stop || !l.st->step_ok) return;
    if (kCal) cam = l.cal->trial;
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
            if (kCal) {
                const double* Wq = l.Wq + 9 * (int64_t)p;
                const double* dq = l.cal->dq;
#pragma unroll
                for (int j = 0; j < 3; ++j) t[j] -= (Wq[j] * dq[0] + Wq[3 + j] * dq[1]) + Wq[6 + j] * dq[2];
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

// The calibrating call's: also the current camera as K_out (the input K after a bad start or a bad index)
__global__ void bundle_finish_calibrated_kernel(Lm w, sfm_bundle_info* __restrict__ info, double* __restrict__ K_out) {
    sfmlm::write_info(w.st, info);
    const PnPCamera& k = w.cal->cam;
    const double K[9] = {k.k00, k.k01, k.k02, k.k10, k.k11, k.k12, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) K_out[i] = K[i];
}

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
    int refine;      // kCal: SFM_BUNDLE_REFINE_* bits and where the refined camera matrix goes
    double* K_out;
};

// Enqueue the whole call; kRobust picks the kernels of a non-squared loss (w.lm.loss), kCal those that refine intrinsics.
template <bool kRobust, bool kCal = false>
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
    if (kCal) hipLaunchKernelGGL(bundle_calib_init_kernel, dim3(1), dim3(1), 0, st, w.lm.cal, cam, job.refine);
    w.pos_c = sfmlm::launch_orders(obs, M, C, P, core, st);
    auto linearize = [&]() {
        hipLaunchKernelGGL((sfmlm::linearize_kernel<true, kRobust, kCal>), dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam,
                           poses_out, points_out, (int)C, w.lm, w.W);
        if (F > 0)
            hipLaunchKernelGGL((sfmlm::camera_kernel<kRobust, kCal>), dim3((unsigned)F), dim3(kThreads), 0, st, obs, cam, poses_out,
                               points_out, w.lm);
    };
    linearize();
    hipLaunchKernelGGL(sfmlm::start_kernel<kThreads>, dim3(1), dim3(kThreads), 0, st, pblocks, f, anchor, max_steps, poses_out,
                       w.lm);
    for (int step = 0; step < max_steps; ++step) {
        linearize();
        hipLaunchKernelGGL(sfmlm::point_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, w.lm);
        if (pairs > 0) hipLaunchKernelGGL(bundle_schur_kernel<kCal>, dim3(pairs), dim3(kThreads), 0, st, F, w);
        if (kCal) hipLaunchKernelGGL(bundle_border_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, w.lm);
        if (F <= kLdsFree)
            hipLaunchKernelGGL((bundle_solve_kernel<true, kCal>), dim3(1), dim3(kSolveThreads), 0, st, F, (int)C, poses_out, w,
                               pblocks);
        else
            hipLaunchKernelGGL((bundle_solve_kernel<false, kCal>), dim3(1), dim3(kSolveThreads), 0, st, F, (int)C, poses_out, w,
                               pblocks);
        hipLaunchKernelGGL((bundle_trial_kernel<kRobust, kCal>), dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, points_out,
                           (int)C, w);
        hipLaunchKernelGGL(sfmlm::decide_kernel<kThreads>, dim3(1), dim3(kThreads), 0, st, pblocks, anchor, max_steps, w.lm);
        hipLaunchKernelGGL(sfmlm::commit_kernel<kCal>, dim3(icgrid), dim3(kThreads), 0, st, (int)P, (int)C, anchor, poses_out,
                           points_out, w.lm);
    }
    if (kCal) hipLaunchKernelGGL(bundle_finish_calibrated_kernel, dim3(1), dim3(1), 0, st, w.lm, job.info, job.K_out);
    else hipLaunchKernelGGL(bundle_finish_kernel, dim3(1), dim3(1), 0, st, w.lm, job.info);
    return check_launch("sfm_bundle_adjust");
}

// Both doors of the adjuster: refine = 0 is sfm_bundle_adjust_ex; else the SFM_BUNDLE_REFINE_* bits of a calibrating call
// (checked by the caller) and K_out.  Every check before the first launch: a refused call has enqueued nothing.
int adjust(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed, const double* poses_in,
           const double* points_in, const int32_t* camera_index, const int32_t* point_index, const double* pixels,
           int max_steps, double* poses_out, double* points_out, sfm_bundle_info* info, void* workspace,
           int64_t workspace_bytes, void* stream, const sfm_bundle_options* options, int refine, double* K_out) {
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
    if ((refine & SFM_BUNDLE_REFINE_FOCAL) && cam.k00 == 0.0)
        return fail(SFM_EINVAL, "sfm_bundle_adjust_calibrated: K[0,0] is zero: the focal length cannot be refined");
    if (!fixed) return fail(SFM_EINVAL, "sfm_bundle_adjust: null pointer (fixed)");
    uint64_t mask = 0;
    for (int64_t c = 0; c < cameras; ++c)
        if (fixed[c]) mask |= 1ull << c;
    if (mask == 0) return fail(SFM_EINVAL, "sfm_bundle_adjust: at least one camera must be fixed");
    if (!poses_in || !poses_out || !info || !workspace || (points > 0 && (!points_in || !points_out)) ||
        (observations > 0 && (!camera_index || !point_index || !pixels)) || (refine && !K_out))
        return fail(SFM_EINVAL, "sfm_bundle_adjust: null pointer");
    const int64_t C = cameras, P = points, M = observations;
    Ws w;
    sfmlm::Core core;
    if (workspace_bytes < carve((uintptr_t)workspace, C, P, M, &w, &core, refine != 0))
        return fail(SFM_EINVAL, "sfm_bundle_adjust: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_bundle_adjust: workspace must be 16-byte aligned");

    w.lm.loss = loss;
    const Job job{cam, C, P, M, mask, poses_in, points_in, Obs{camera_index, point_index, pixels}, max_steps, poses_out, points_out,
                  info, (hipStream_t)stream, refine, K_out};
    const bool robust = loss.kind != SFM_BUNDLE_LOSS_SQUARED;
    if (refine) return robust ? enqueue<true, true>(job, w, core) : enqueue<false, true>(job, w, core);
    return robust ? enqueue<true>(job, w, core) : enqueue<false>(job, w, core);
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

int64_t sfm_bundle_calibrated_workspace_bytes(int64_t cameras, int64_t points, int64_t observations) {
    if (sfm_bundle_workspace_bytes(cameras, points, observations) < 0) return -1;
    Ws w;
    sfmlm::Core core;
    return carve(0, cameras, points, observations, &w, &core, true);
}

int sfm_bundle_adjust_ex(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                         const double* poses_in, const double* points_in, const int32_t* camera_index,
                         const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                         double* points_out, sfm_bundle_info* info, void* workspace, int64_t workspace_bytes, void* stream,
                         const sfm_bundle_options* options) {
    return adjust(K, cameras, points, observations, fixed, poses_in, points_in, camera_index, point_index, pixels, max_steps,
                  poses_out, points_out, info, workspace, workspace_bytes, stream, options, 0, nullptr);
}

int sfm_bundle_adjust_calibrated(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                                 const double* poses_in, const double* points_in, const int32_t* camera_index,
                                 const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                                 double* points_out, sfm_bundle_info* info, double* K_out, void* workspace,
                                 int64_t workspace_bytes, void* stream, const sfm_bundle_calibration_options* options) {
    if (!options) return fail(SFM_EINVAL, "sfm_bundle_adjust_calibrated: null pointer (options)");
    if (options->refine < 1 || options->refine > (SFM_BUNDLE_REFINE_FOCAL | SFM_BUNDLE_REFINE_PRINCIPAL_POINT) ||
        options->reserved != 0)
        return fail(SFM_EINVAL, "sfm_bundle_adjust_calibrated: options need refine in 1..3 and reserved = 0");
    return adjust(K, cameras, points, observations, fixed, poses_in, points_in, camera_index, point_index, pixels, max_steps,
                  poses_out, points_out, info, workspace, workspace_bytes, stream, &options->loss, options->refine, K_out);
}

int sfm_bundle_adjust(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                      const double* poses_in, const double* points_in, const int32_t* camera_index,
                      const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                      double* points_out, sfm_bundle_info* info, void* workspace, int64_t workspace_bytes, void* stream) {
    return sfm_bundle_adjust_ex(K, cameras, points, observations, fixed, poses_in, points_in, camera_index, point_index, pixels,
                                max_steps, poses_out, points_out, info, workspace, workspace_bytes, stream, nullptr);
}

}  // extern "C"
