// Bundle adjustment with an iterative Schur solver: the Levenberg-Marquardt loop of csrc/sfm_bundle_lm.h
// over any number of cameras, with the damped reduced camera system S* dc = b solved by conjugate gradients preconditioned
// with S*'s 6 x 6 diagonal blocks (block Jacobi).  S* = U* - W V*^-1 W^T is applied matrix-free and never formed
// (the NumPy oracle is tests/bundle_pcg_oracle.py).  fp64 throughout; off unless asked for.
//
// The Jacobians are recomputed from the pose and the point wherever W = Jc^T Jp is needed, instead of storing W (144 B
// per observation): W^T x = Jp^T (Jc x) and W y = Jc^T (Jp y).  A pass then reads the indices, the point and the pose.
//
// Set-up, once per call: the free cameras' slots (from the host), the point-major and the camera-major orders of
// csrc/sfm_obs_order.h.  Then per LM trial step, every launch reading the LM state first and returning at once after a
// stop:
//   linearize_kernel<false> (after an accepted step)  thread per point: V_p, g_p and the cost of its observations
//   camera_kernel           (after an accepted step)  block per free camera: U_c and g_c over its camera-major list
//   point_kernel            thread per point: V_p* = V_p + lambda diag V_p and its inverse
//   pcg_precond_kernel      block per free camera: M_c = U*_c - sum_p W_cp V_p*^-1 W_cp^T, b_c, and M_c^-1 by Cholesky
//   pcg_cg_init_kernel      one workgroup: x = 0, r = b, z = M^-1 r, p = z
//   per CG iteration:       pcg_cg_point_kernel  (thread per point: y_p = V_p*^-1 sum W^T p_c)
//                           pcg_cg_camera_kernel (block per free camera: q_c = U*_c p_c - sum W y_p, and p_c . q_c)
//                           pcg_cg_update_kernel (one workgroup: alpha, x, r, z, rho, beta, p and the stop of CG)
//   pcg_apply_kernel        one workgroup: finish_step (the camera steps, the trial poses, the camera part of |delta|, |x|)
//   pcg_trial_kernel        thread per point: back-substitution dX_p, the trial point, its observations' trial cost
//   decide_kernel<1024>     one workgroup: accept / reject, lambda, the gauge scale, stops
//   commit_kernel           an accepted trial becomes the current estimate (rescaled when one camera is fixed)
// The host reads two flags (LM stop, CG done) from pinned memory once per LM step and once per chunk of kCgChunk CG
// iterations, and enqueues no more work after a stop.  The device state alone decides the result: every kernel also
// returns at once after a stop, so the reads only save launches.  No floating-point atomics anywhere: every sum runs in
// an order fixed by the sizes alone, so a call is bit-reproducible.
//
// A robust loss (csrc/sfm_loss.h) runs the kRobust = true forms of the kernels that see a residual or a
// Jacobian.  The kernels that recompute Jc and Jp without a residual (the preconditioner, both CG passes, the trial's
// back-substitution) read sqrt(w) from lm.sw, which the linearisation stored once per point-major position (8 B per
// observation, in the workspace of a non-squared call only); the camera-major ones reach it through pos_c.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "sfm_bundle_lm.h"
#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_pnp.h"

namespace {

using sfm::block_sum;
using sfmhost::check_launch;
using sfmhost::fail;
using sfmlm::kThreads;
using sfmlm::Lm;
using sfmlm::Obs;
using sfmlm::sym3;
using sfmlm::upper6;
using sfmpnp::camera_from;
using sfmpnp::jacobians;
using sfmpnp::pnp_score;
using sfmpnp::PnPCamera;

constexpr int kOneGroup = 1024;       // the one-workgroup kernels
constexpr int kCgChunk = 10;          // CG iterations enqueued between two reads of the flags

static_assert(sizeof(sfm_bundle_pcg_info) == 40, "sfm_bundle_pcg_info layout is part of the ABI");

// The LM state and the CG state after it: written by one thread of the one-workgroup kernels, read by every launch after it.
struct State {
    sfmlm::State lm;
    int32_t cg_done;        // right after lm.stop: the host reads both at once
    int32_t cg_fail;        // this step is rejected (a failed factorisation or a breakdown at k = 0)
    int32_t cg_k, cg_total, cg_max;
    int32_t pad;
    double rho, tol2;       // CG: r^T z, and tol^2 |b|^2
};
static_assert(offsetof(State, cg_done) == offsetof(State, lm) + offsetof(sfmlm::State, stop) + sizeof(int32_t),
              "the host reads {stop, cg_done} as one pair");

struct Ws {
    Lm lm;
    State* st;
    const int32_t* pos_c;   // camera-major position -> point-major position (set after the orders are enqueued)
    double *y, *Minv, *b, *x, *r, *z, *p, *q, *part;
};

// The workspace from `base` (0: sizes only); its size in bytes.
int64_t carve(uintptr_t base, int64_t C, int64_t P, int64_t M, int64_t F, bool robust, Ws* w, sfmlm::Core* core) {
    sfmlm::Carver k{base, 0};
    w->st = k.take<State>(1);
    *core = sfmlm::carve_core(k, C, P, M, F, &w->st->lm);
    w->lm = core->lm;
    w->y = k.take<double>(3 * P);
    w->Minv = k.take<double>(36 * F);
    w->b = k.take<double>(6 * F);
    w->x = k.take<double>(6 * F);
    w->r = k.take<double>(6 * F);
    w->z = k.take<double>(6 * F);
    w->p = k.take<double>(6 * F);
    w->q = k.take<double>(6 * F);
    w->part = k.take<double>(F);
    w->pos_c = nullptr;
    if (robust) w->lm.sw = k.take<double>(M);   // last: the squared layout and size stay as they are
    return k.at;
}

// W^T d = Jp^T (Jc d) (3) and W y = Jc^T (Jp y) (6)
SFM_DEVICE void wt_times(const double (&Jc)[2][6], const double (&Jp)[2][3], const double* d, double (&out)[3]) {
    double e[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) e[q] = ((((Jc[q][0] * d[0] + Jc[q][1] * d[1]) + Jc[q][2] * d[2]) + Jc[q][3] * d[3]) +
                                        Jc[q][4] * d[4]) + Jc[q][5] * d[5];
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = Jp[0][j] * e[0] + Jp[1][j] * e[1];
}

SFM_DEVICE void w_times(const double (&Jc)[2][6], const double (&Jp)[2][3], const double* y, double (&out)[6]) {
    double e[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) e[q] = (Jp[q][0] * y[0] + Jp[q][1] * y[1]) + Jp[q][2] * y[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = Jc[0][i] * e[0] + Jc[1][i] * e[1];
}

// The state; the free cameras' list from the slots (slot[c] = -1 for a fixed camera)
__global__ __launch_bounds__(kThreads) void pcg_init_kernel(int C, Ws w) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c == 0) {
        *w.st = State{};
        sfmlm::init_state(w.lm.st);
    }
    if (c < C && w.lm.slot[c] >= 0) w.lm.freec[w.lm.slot[c]] = c;
}

// ------------------------------------------------------------------------------------------------------------------------
// One LM trial step: the preconditioner and the right-hand side.
// ------------------------------------------------------------------------------------------------------------------------
// U*_c = U_c + lambda diag U_c (full 6 x 6)
SFM_DEVICE void damped_u(const double* u, double lambda, double (&A)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = u[upper6(i, j)];
#pragma unroll
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + lambda * A[i][i];
}

// Block per free camera (slot s): M_c = U*_c - sum over its observations of moving points of W V_p*^-1 W^T, b_c = -g_c +
// sum W V_p*^-1 g_p, and M_c^-1 (full 36) from its Cholesky factor (sfm_lm.h).  A pivot <= 0 or not finite marks the step
// as failed.
template <bool kRobust>
__global__ __launch_bounds__(kThreads) void pcg_precond_kernel(PnPCamera cam, const double* __restrict__ poses,
                                                               const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave * 27];
    __shared__ double total[27];
    if (w.st->lm.stop || w.st->lm.fail) return;
    const sfmlm::Chunk ch = sfmlm::camera_chunk(w.lm);
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * (int64_t)ch.c + k];
    double a[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) a[k] = 0.0;
    for (int i = ch.i0; i < ch.i1; ++i) {
        const int64_t p = w.lm.pt_c[i];
        if (w.lm.off_p[p + 1] - w.lm.off_p[p] < 2) continue;
        double Jc[2][6], Jp[2][3];
        if (!jacobians(m, cam, points[3 * p], points[3 * p + 1], points[3 * p + 2], Jc, Jp)) continue;
        if (kRobust) sfmloss::scale(w.lm.sw[w.pos_c[i]], Jc, Jp);
        double Wm[6][3], Vi[3][3], Y[6][3];
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int j = 0; j < 3; ++j) Wm[x][j] = Jc[0][x] * Jp[0][j] + Jc[1][x] * Jp[1][j];
        sym3(w.lm.Vi + 6 * p, Vi);
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int j = 0; j < 3; ++j) Y[x][j] = (Wm[x][0] * Vi[0][j] + Wm[x][1] * Vi[1][j]) + Wm[x][2] * Vi[2][j];
        const double* g = w.lm.gp + 3 * p;
#pragma unroll
        for (int x = 0; x < 6; ++x) {
#pragma unroll
            for (int y = x; y < 6; ++y) a[upper6(x, y)] += (Y[x][0] * Wm[y][0] + Y[x][1] * Wm[y][1]) + Y[x][2] * Wm[y][2];
            a[21 + x] += (Y[x][0] * g[0] + Y[x][1] * g[1]) + Y[x][2] * g[2];
        }
    }
    block_sum<27, kThreads>(a, part, total);
    if (threadIdx.x != 0) return;
    const int s = blockIdx.x;
    double A[6][6];
    damped_u(w.lm.U + 21 * (int64_t)ch.c, w.st->lm.lambda, A);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = A[i][j] - total[upper6(i, j)];
#pragma unroll
    for (int i = 0; i < 6; ++i) w.b[6 * (int64_t)s + i] = -w.lm.gc[6 * (int64_t)ch.c + i] + total[21 + i];
    double L[6][6], inv[6][6];
    if (!sfmlm::factor<6>(A, 0.0, L)) {
        w.st->lm.fail = 1;
        return;
    }
    sfmlm::inverse<6>(L, inv);
    double* out = w.Minv + 36 * (int64_t)s;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) out[6 * i + j] = inv[i][j];
}

// z_s = M_s^-1 r_s
SFM_DEVICE void precondition(const double* Minv, const double* r, double* z) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) v += Minv[6 * i + j] * r[j];
        z[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Preconditioned conjugate gradients on S* dc = b.
// ------------------------------------------------------------------------------------------------------------------------
// One workgroup: x = 0, r = b, z = M^-1 r, p = z, rho = r.z, tol2 = tol^2 |b|^2.  A failed factorisation or a non-finite
// rho or |b|^2 rejects the step.  Sets cg_fail and cg_done afresh on every step that runs.
__global__ __launch_bounds__(kOneGroup) void pcg_cg_init_kernel(int F, double tol, Ws w) {
    __shared__ double part[kOneGroup / kWave * 2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->lm.stop) return;
    const bool failed = st->lm.fail;
    __syncthreads();   // every thread has read the state before thread 0 writes it
    if (threadIdx.x == 0) {
        st->lm.need_lin = 0;   // the linearisation kernels of this step have run
        st->cg_k = 0;
    }
    if (failed) {
        if (threadIdx.x == 0) {
            st->cg_fail = 1;
            st->cg_done = 1;
        }
        return;
    }
    double v[2] = {0.0, 0.0};   // r.z | b.b
    for (int s = threadIdx.x; s < F; s += kOneGroup) {
        const double* b = w.b + 6 * (int64_t)s;
        double z[6];
        precondition(w.Minv + 36 * (int64_t)s, b, z);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            w.x[6 * (int64_t)s + k] = 0.0;
            w.r[6 * (int64_t)s + k] = b[k];
            w.z[6 * (int64_t)s + k] = z[k];
            w.p[6 * (int64_t)s + k] = z[k];
            v[0] += b[k] * z[k];
            v[1] += b[k] * b[k];
        }
    }
    block_sum<2, kOneGroup>(v, part, total);
    if (threadIdx.x != 0) return;
    const bool bad = !isfinite(total[0]) || !isfinite(total[1]);
    st->rho = total[0];
    st->tol2 = tol * tol * total[1];
    st->cg_fail = bad;
    st->cg_done = bad || total[1] <= st->tol2;
}

// Thread per point: y_p = V_p*^-1 sum over its observations by free cameras of W^T p_c (0 for a point that does not move)
template <bool kRobust>
__global__ __launch_bounds__(kThreads) void pcg_cg_point_kernel(int P, PnPCamera cam, const double* __restrict__ poses,
                                                                const double* __restrict__ points, Ws w) {
    if (w.st->lm.stop || w.st->cg_done) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int q0 = w.lm.off_p[p], q1 = w.lm.off_p[p + 1];
    double t[3] = {0.0, 0.0, 0.0};
    if (q1 - q0 >= 2) {
        const double X = points[3 * (int64_t)p], Y = points[3 * (int64_t)p + 1], Z = points[3 * (int64_t)p + 2];
        for (int q = q0; q < q1; ++q) {
            const int c = w.lm.camp[q], s = w.lm.slot[c];
            if (s < 0) continue;
            double Jc[2][6], Jp[2][3], d[3];
            if (!jacobians(poses + 12 * (int64_t)c, cam, X, Y, Z, Jc, Jp)) continue;
            if (kRobust) sfmloss::scale(w.lm.sw[q], Jc, Jp);
            wt_times(Jc, Jp, w.p + 6 * (int64_t)s, d);
#pragma unroll
            for (int j = 0; j < 3; ++j) t[j] += d[j];
        }
        double Vi[3][3];
        sym3(w.lm.Vi + 6 * (int64_t)p, Vi);
        double yv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) yv[i] = (Vi[i][0] * t[0] + Vi[i][1] * t[1]) + Vi[i][2] * t[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = yv[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) w.y[3 * (int64_t)p + i] = t[i];
}

// Block per free camera (slot s): q_s = U*_c p_s - sum over its observations of W y_p, and part_s = p_s . q_s
template <bool kRobust>
__global__ __launch_bounds__(kThreads) void pcg_cg_camera_kernel(PnPCamera cam, const double* __restrict__ poses,
                                                                 const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave * 6];
    __shared__ double total[6];
    if (w.st->lm.stop || w.st->cg_done) return;
    const sfmlm::Chunk ch = sfmlm::camera_chunk(w.lm);
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * (int64_t)ch.c + k];
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = ch.i0; i < ch.i1; ++i) {
        const int64_t p = w.lm.pt_c[i];
        double Jc[2][6], Jp[2][3], e[6];
        if (!jacobians(m, cam, points[3 * p], points[3 * p + 1], points[3 * p + 2], Jc, Jp)) continue;
        if (kRobust) sfmloss::scale(w.lm.sw[w.pos_c[i]], Jc, Jp);
        w_times(Jc, Jp, w.y + 3 * p, e);
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] += e[k];
    }
    block_sum<6, kThreads>(a, part, total);
    if (threadIdx.x != 0) return;
    const int s = blockIdx.x;
    double A[6][6];
    damped_u(w.lm.U + 21 * (int64_t)ch.c, w.st->lm.lambda, A);
    const double* pv = w.p + 6 * (int64_t)s;
    double pq = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) v += A[i][j] * pv[j];
        v -= total[i];
        w.q[6 * (int64_t)s + i] = v;
        pq += pv[i] * v;
    }
    w.part[s] = pq;
}

// One workgroup: alpha = rho / p.q, x += alpha p, r -= alpha q, z = M^-1 r, rho' = r.z, beta = rho' / rho, p = z + beta p.
// CG stops at |r|^2 <= tol2, at max_iterations, or at a breakdown (p.q <= 0 or a non-finite scalar; the iterate reached so
// far is the step, and a breakdown at k = 0 rejects it).
__global__ __launch_bounds__(kOneGroup) void pcg_cg_update_kernel(int F, int max_iterations, Ws w) {
    __shared__ double part[kOneGroup / kWave * 2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->lm.stop || st->cg_done) return;
    const double rho = st->rho, tol2 = st->tol2;
    const int k = st->cg_k;
    double v[2] = {0.0, 0.0};
    for (int s = threadIdx.x; s < F; s += kOneGroup) v[0] += w.part[s];
    block_sum<2, kOneGroup>(v, part, total);   // its barriers order every read of the state above before the writes below
    const double pq = total[0];
    const double alpha = rho / pq;
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(alpha)) {
        if (threadIdx.x == 0) {
            st->cg_done = 1;
            if (k == 0) st->cg_fail = 1;
        }
        return;
    }
    v[0] = v[1] = 0.0;   // r.z | r.r
    for (int s = threadIdx.x; s < F; s += kOneGroup) {
        double* x = w.x + 6 * (int64_t)s;
        double* r = w.r + 6 * (int64_t)s;
        double* z = w.z + 6 * (int64_t)s;
        const double* p = w.p + 6 * (int64_t)s;
        const double* q = w.q + 6 * (int64_t)s;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            x[i] = x[i] + alpha * p[i];
            r[i] = r[i] - alpha * q[i];
        }
        precondition(w.Minv + 36 * (int64_t)s, r, z);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            v[0] += r[i] * z[i];
            v[1] += r[i] * r[i];
        }
    }
    block_sum<2, kOneGroup>(v, part, total);
    const double rz = total[0], rr = total[1];
    const bool broke = !isfinite(rz) || !isfinite(rr);
    const double beta = rz / rho;
    const bool done = broke || rr <= tol2 || k + 1 == max_iterations;
    if (!done)
        for (int s = threadIdx.x; s < F; s += kOneGroup) {
            double* p = w.p + 6 * (int64_t)s;
            const double* z = w.z + 6 * (int64_t)s;
#pragma unroll
            for (int i = 0; i < 6; ++i) p[i] = z[i] + beta * p[i];
        }
    if (threadIdx.x == 0) {
        st->cg_k = k + 1;
        st->rho = rz;
        st->cg_done = done;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// The trial step and the decision.
// ------------------------------------------------------------------------------------------------------------------------
// One workgroup: the step is rejected after a CG failure or when a camera step is not finite; else the camera steps dc
// (by camera, 0 for a fixed one) and the trial poses (finish_step).
__global__ __launch_bounds__(kOneGroup) void pcg_apply_kernel(int C, const double* __restrict__ poses, Ws w) {
    State* st = w.st;
    if (st->lm.stop) return;
    const int k = st->cg_k;
    bool finite = true;
    for (int c = threadIdx.x; c < C; c += kOneGroup) {
        const int s = w.lm.slot[c];
        if (s < 0) continue;
        for (int i = 0; i < 6; ++i) finite = finite && isfinite(w.x[6 * (int64_t)s + i]);
    }
    const bool ok = __syncthreads_and(finite) && !st->cg_fail;
    sfmlm::finish_step<kOneGroup>(ok, w.x, C, poses, w.lm);
    if (threadIdx.x != 0) return;
    st->cg_total += k;
    st->cg_max = max(st->cg_max, k);
}

// Thread per point: dX_p = V_p*^-1 (-g_p - sum over its free-camera observations of W^T dc), the trial point, the trial
// cost of its observations (kRobust: the sum of rho) and its share of |delta|^2 and |x|^2; partials per block.
template <bool kRobust>
__global__ __launch_bounds__(kThreads) void pcg_trial_kernel(Obs obs, int P, PnPCamera cam, const double* __restrict__ poses,
                                                             const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave * 3];
    __shared__ double total[3];
    if (w.st->lm.stop || !w.st->lm.step_ok) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};   // cost | |dX|^2 | |X|^2
    if (p < P) {
        double X[3] = {points[3 * (int64_t)p], points[3 * (int64_t)p + 1], points[3 * (int64_t)p + 2]};
        const int q0 = w.lm.off_p[p], q1 = w.lm.off_p[p + 1];
        if (q1 - q0 >= 2) {
            double t[3] = {-w.lm.gp[3 * (int64_t)p], -w.lm.gp[3 * (int64_t)p + 1], -w.lm.gp[3 * (int64_t)p + 2]};
            for (int q = q0; q < q1; ++q) {
                const int c = w.lm.camp[q];
                if (w.lm.slot[c] < 0) continue;
                double Jc[2][6], Jp[2][3], d[3];
                if (!jacobians(poses + 12 * (int64_t)c, cam, X[0], X[1], X[2], Jc, Jp)) continue;
                if (kRobust) sfmloss::scale(w.lm.sw[q], Jc, Jp);
                wt_times(Jc, Jp, w.lm.dc + 6 * (int64_t)c, d);
#pragma unroll
                for (int j = 0; j < 3; ++j) t[j] -= d[j];
            }
            double Vi[3][3];
            sym3(w.lm.Vi + 6 * (int64_t)p, Vi);
            double dX[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) dX[i] = (Vi[i][0] * t[0] + Vi[i][1] * t[1]) + Vi[i][2] * t[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a[1] += dX[i] * dX[i];
                a[2] += X[i] * X[i];
                X[i] += dX[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) w.lm.tpts[3 * (int64_t)p + i] = X[i];
        for (int q = q0; q < q1; ++q) {
            const int64_t m = w.lm.ord_p[q];
            const double e = pnp_score(w.lm.tpose + 12 * (int64_t)w.lm.camp[q], cam, X[0], X[1], X[2], obs.uv[2 * m], obs.uv[2 * m + 1]);
            a[0] += kRobust ? sfmloss::rho(w.lm.loss, e) : e;
        }
    }
    block_sum<3, kThreads>(a, part, total);
    if (threadIdx.x < 3) w.lm.part[3 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

__global__ void pcg_finish_kernel(Ws w, sfm_bundle_pcg_info* __restrict__ info) {
    sfmlm::write_info(w.lm.st, info);
    info->cg_iterations = w.st->cg_total;
    info->cg_max = w.st->cg_max;
}

// The host's copy of the two flags {stop, cg_done}: pinned, one per host thread, allocated on its first call and kept.
int32_t* pinned_flags() {
    thread_local int32_t* flags = nullptr;
    if (!flags && hipHostMalloc(reinterpret_cast<void**>(&flags), 2 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
        flags = nullptr;
    return flags;
}

// A checked call: everything enqueue needs.
struct Job {
    PnPCamera cam;
    int64_t C, P, M, F;
    const int32_t* slot;   // host
    int first_fixed, anchor;
    const double *poses_in, *points_in;
    Obs obs;
    int max_steps, max_cg_iterations;
    double cg_tolerance;
    double *poses_out, *points_out;
    sfm_bundle_pcg_info* info;
    int32_t* flags;
    hipStream_t st;
};

// Enqueue the call step by step; kRobust picks the kernels of a non-squared loss (w.lm.loss, w.lm.sw).
template <bool kRobust>
int enqueue(const Job& job, Ws& w, const sfmlm::Core& core) {
    const PnPCamera& cam = job.cam;
    const int64_t C = job.C, P = job.P, M = job.M, F = job.F;
    const double *poses_in = job.poses_in, *points_in = job.points_in;
    double *poses_out = job.poses_out, *points_out = job.points_out;
    const int max_steps = job.max_steps, max_cg_iterations = job.max_cg_iterations, anchor = job.anchor;
    const double cg_tolerance = job.cg_tolerance;
    int32_t* flags = job.flags;
    hipStream_t st = job.st;
    const Obs& obs = job.obs;
    const unsigned pgrid = sfmhost::grid_for(P, kThreads), cgrid = sfmhost::grid_for(C, kThreads);
    const unsigned icgrid = sfmhost::grid_for(P > C ? P : C, kThreads);
    const int pblocks = (int)((P + kThreads - 1) / kThreads);
    // reads {stop, cg_done} into the pinned flags (synchronises the stream)
    auto read_flags = [&]() -> int {
        if (hipMemcpyAsync(flags, &w.st->lm.stop, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return check_launch("sfm_bundle_adjust_pcg: read the flags");
        return SFM_OK;
    };

    // the output starts as the input; the slots come from the host; the point counters start at zero
    if (poses_out != poses_in && hipMemcpyAsync(poses_out, poses_in, 8 * 12 * C, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return check_launch("sfm_bundle_adjust_pcg: copy poses");
    if (P > 0 && points_out != points_in &&
        hipMemcpyAsync(points_out, points_in, 8 * 3 * P, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return check_launch("sfm_bundle_adjust_pcg: copy points");
    if (hipMemcpyAsync(w.lm.slot, job.slot, 4 * C, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(w.lm.off_p, 0, 4 * (P + 1), st) != hipSuccess)
        return check_launch("sfm_bundle_adjust_pcg: set up the workspace");
    hipLaunchKernelGGL(pcg_init_kernel, dim3(cgrid), dim3(kThreads), 0, st, (int)C, w);
    w.pos_c = sfmlm::launch_orders(obs, M, C, P, core, st);
    auto linearize = [&]() {
        hipLaunchKernelGGL((sfmlm::linearize_kernel<false, kRobust>), dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam,
                           poses_out, points_out, (int)C, w.lm, nullptr);
        if (F > 0)
            hipLaunchKernelGGL(sfmlm::camera_kernel<kRobust>, dim3((unsigned)F), dim3(kThreads), 0, st, obs, cam, poses_out,
                               points_out, w.lm);
    };
    linearize();
    hipLaunchKernelGGL(sfmlm::start_kernel<kOneGroup>, dim3(1), dim3(kOneGroup), 0, st, pblocks, job.first_fixed, anchor,
                       max_steps, poses_out, w.lm);
    for (int step = 0; step < max_steps; ++step) {
        int rc2 = read_flags();   // also the point after which the host slots may go
        if (rc2 != SFM_OK) return rc2;
        if (flags[0]) break;
        linearize();
        hipLaunchKernelGGL(sfmlm::point_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, w.lm);
        if (F > 0)
            hipLaunchKernelGGL(pcg_precond_kernel<kRobust>, dim3((unsigned)F), dim3(kThreads), 0, st, cam, poses_out, points_out,
                               w);
        hipLaunchKernelGGL(pcg_cg_init_kernel, dim3(1), dim3(kOneGroup), 0, st, (int)F, cg_tolerance, w);
        for (int k0 = 0; F > 0 && k0 < max_cg_iterations; k0 += kCgChunk) {
            if (k0 > 0) {
                rc2 = read_flags();
                if (rc2 != SFM_OK) return rc2;
                if (flags[0] || flags[1]) break;
            }
            for (int k = k0; k < max_cg_iterations && k < k0 + kCgChunk; ++k) {
                hipLaunchKernelGGL(pcg_cg_point_kernel<kRobust>, dim3(pgrid), dim3(kThreads), 0, st, (int)P, cam, poses_out,
                                   points_out, w);
                hipLaunchKernelGGL(pcg_cg_camera_kernel<kRobust>, dim3((unsigned)F), dim3(kThreads), 0, st, cam, poses_out,
                                   points_out, w);
                hipLaunchKernelGGL(pcg_cg_update_kernel, dim3(1), dim3(kOneGroup), 0, st, (int)F, max_cg_iterations, w);
            }
        }
        hipLaunchKernelGGL(pcg_apply_kernel, dim3(1), dim3(kOneGroup), 0, st, (int)C, poses_out, w);
        hipLaunchKernelGGL(pcg_trial_kernel<kRobust>, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, poses_out, points_out,
                           w);
        hipLaunchKernelGGL(sfmlm::decide_kernel<kOneGroup>, dim3(1), dim3(kOneGroup), 0, st, pblocks, anchor, max_steps, w.lm);
        hipLaunchKernelGGL(sfmlm::commit_kernel<>, dim3(icgrid), dim3(kThreads), 0, st, (int)P, (int)C, anchor, poses_out,
                           points_out, w.lm);
    }
    hipLaunchKernelGGL(pcg_finish_kernel, dim3(1), dim3(1), 0, st, w, job.info);
    if (max_steps == 0) {   // no read above: the host slots must reach the device before they go
        const int rc2 = read_flags();
        if (rc2 != SFM_OK) return rc2;
    }
    return check_launch("sfm_bundle_adjust_pcg");
}

}  // namespace

extern "C" {

int64_t sfm_bundle_pcg_workspace_bytes_ex(int64_t cameras, int64_t points, int64_t observations,
                                          const sfm_bundle_options* options) {
    sfmloss::Loss loss;
    if (cameras < 1 || points < 0 || observations < 0 || cameras > 0x7FFFFFFF || points > 0x7FFFFFFF ||
        observations > 0x7FFFFFFF || !sfmloss::from_options(options, loss))
        return -1;
    Ws w;
    sfmlm::Core core;
    return carve(0, cameras, points, observations, cameras - 1, loss.kind != SFM_BUNDLE_LOSS_SQUARED, &w, &core);
}

int64_t sfm_bundle_pcg_workspace_bytes(int64_t cameras, int64_t points, int64_t observations) {
    return sfm_bundle_pcg_workspace_bytes_ex(cameras, points, observations, nullptr);
}

int sfm_bundle_adjust_pcg_ex(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                             const double* poses_in, const double* points_in, const int32_t* camera_index,
                             const int32_t* point_index, const double* pixels, int max_steps, int max_cg_iterations,
                             double cg_tolerance, double* poses_out, double* points_out, sfm_bundle_pcg_info* info,
                             void* workspace, int64_t workspace_bytes, void* stream, const sfm_bundle_options* options) {
    // every check before the first launch: a refused call has enqueued nothing
    if (cameras < 1 || points < 0 || observations < 0 || max_steps < 0)
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: bad size");
    if (cameras > 0x7FFFFFFF || points > 0x7FFFFFFF || observations > 0x7FFFFFFF)
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: cameras, points and observations must be below 2^31");
    if (max_cg_iterations < 1) return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: max_cg_iterations must be at least 1");
    if (!(cg_tolerance > 0.0 && cg_tolerance < 1.0))
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: cg_tolerance must be finite and in (0, 1)");
    sfmloss::Loss loss;
    if (!sfmloss::from_options(options, loss))
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: options need a loss in 0..2, reserved = 0 and a loss_scale > 0 with a normal finite square");
    PnPCamera cam;
    const int rc = camera_from(K, cam, "sfm_bundle_adjust_pcg");
    if (rc != SFM_OK) return rc;
    if (!fixed) return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: null pointer (fixed)");
    const int64_t C = cameras, P = points, M = observations;
    std::vector<int32_t> slot((size_t)C);
    int64_t F = 0, first_fixed = -1, first_free = -1;
    for (int64_t c = 0; c < C; ++c) {
        if (fixed[c]) {
            slot[(size_t)c] = -1;
            if (first_fixed < 0) first_fixed = c;
        } else {
            if (first_free < 0) first_free = c;
            slot[(size_t)c] = (int32_t)F++;
        }
    }
    if (F == C) return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: at least one camera must be fixed");
    if (!poses_in || !poses_out || !info || !workspace || (points > 0 && (!points_in || !points_out)) ||
        (observations > 0 && (!camera_index || !point_index || !pixels)))
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: null pointer");
    const bool robust = loss.kind != SFM_BUNDLE_LOSS_SQUARED;
    Ws w;
    sfmlm::Core core;
    if (workspace_bytes < carve((uintptr_t)workspace, C, P, M, F, robust, &w, &core))
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: workspace must be 16-byte aligned");
    int32_t* flags = pinned_flags();
    if (!flags) return fail(SFM_EHIP, "sfm_bundle_adjust_pcg: no pinned host memory for the flags");
    w.lm.loss = loss;
    const int anchor = C - F == 1 && F > 0 ? (int)first_free : -1;   // one fixed camera: the gauge anchor
    const Job job{cam, C, P, M, F, slot.data(), (int)first_fixed, anchor, poses_in, points_in,
                  Obs{camera_index, point_index, pixels}, max_steps, max_cg_iterations, cg_tolerance, poses_out, points_out,
                  info, flags, (hipStream_t)stream};
    return robust ? enqueue<true>(job, w, core) : enqueue<false>(job, w, core);
}

int sfm_bundle_adjust_pcg(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                          const double* poses_in, const double* points_in, const int32_t* camera_index,
                          const int32_t* point_index, const double* pixels, int max_steps, int max_cg_iterations,
                          double cg_tolerance, double* poses_out, double* points_out, sfm_bundle_pcg_info* info,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    return sfm_bundle_adjust_pcg_ex(K, cameras, points, observations, fixed, poses_in, points_in, camera_index, point_index,
                                    pixels, max_steps, max_cg_iterations, cg_tolerance, poses_out, points_out, info, workspace,
                                    workspace_bytes, stream, nullptr);
}

}  // extern "C"
