// The Levenberg-Marquardt core of both bundle adjusters: sfm_bundle.hip (dense Schur solve, at most
// 64 cameras) and sfm_bundle_pcg.hip (conjugate gradients, any camera count).  Here: the LM state and the workspace
// arrays both use, the linearisation, the damped point blocks, the start, the accept / reject decision, the commit and
// the info record.  Each adjuster adds only the solve of its damped reduced camera system, which ends in finish_step.
// The LM constants, the step rules and the small SPD solves are those of every LM loop of the library: csrc/sfm_lm.h.
//
// Every launch reads the LM state in the workspace first and returns at once after a stop.  Cameras are named by slots:
// slot[c] is camera c's index among the free cameras (-1 for a fixed one), freec[s] the camera of slot s.  The gauge's
// fixed camera f and anchor a (the lowest free camera when exactly one camera is fixed, else a = -1) come from the host.
// No floating-point atomics anywhere: every sum runs in an order fixed by the sizes alone.
//
// The kernels that see a residual or a Jacobian take the loss (csrc/sfm_loss.h) as a template parameter:
// kRobust = false is the squared loss and compiles to the code it was before there was a choice; kRobust = true reads the
// launch-uniform Lm::loss, sums rho instead of e and multiplies r, Jc and Jp by sqrt(w).
//
// kCal (the dense adjuster's calibrating call; false everywhere else and then the code it was before) refines
// up to three intrinsics shared by all cameras: the camera is Lm::cal's, not the launch argument, and the kernels add the
// blocks of Jq = dw / d(f, cx, cy): U_qq and g_q, U_cq per camera, W_qp per point.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_lm.h"
#include "sfm_loss.h"
#include "sfm_math.h"
#include "sfm_obs_order.h"
#include "sfm_pnp.h"

namespace sfmlm {

using sfmpnp::PnPCamera;

constexpr int kThreads = 256;      // point-parallel and per-camera kernels
constexpr int kLdsCameras = 64;    // linearize_kernel<true> stages this many poses in LDS (the dense path's limit)

// The LM state: written by one thread of the one-workgroup kernels, read by every launch after it.
struct State {
    double lambda, cost, initial_cost, scale;
    double c0[3], dist;     // gauge: the fixed camera's centre and the anchor camera's distance from it
    double dn_c, xn_c;      // the free cameras' share of |delta|^2 and |x|^2 of this trial step
    int32_t steps, accepted, status;
    int32_t need_lin;       // the current estimate has no linearisation yet (start, or an accepted step)
    int32_t step_ok;        // the damped system was solved and the step is finite
    int32_t commit;         // this step's trial was accepted
    int32_t fail;           // a damped block did not factor (any thread may set it)
    int32_t bad;            // an index is out of range (set by the point order's count kernel)
    int32_t pad;
    int32_t stop;           // last, no padding after it: a state that starts with this one can keep a flag beside it
};
static_assert(offsetof(State, stop) + sizeof(int32_t) == sizeof(State), "stop is the last word of State");

// The calibrating call's cameras and intrinsics step.  A trial step scales the 2 x 2 block of K by (f + df) / f, f = k00
// (a zero entry stays zero), and moves (k02, k12) by (dcx, dcy).
struct Calib {
    PnPCamera cam, trial;   // of the current estimate, of the trial step
    double dq[3];           // the trial step of (f, cx, cy); 0 for a held intrinsic
    int32_t refine, pad;    // SFM_BUNDLE_REFINE_* bits
};

// The observations: camera and point index, pixel.
struct Obs {
    const int32_t* cam;
    const int32_t* pt;
    const double* uv;
};

// The workspace arrays of the core.
struct Lm {
    State* st;
    int32_t *slot, *freec;
    int32_t *off_p, *ord_p, *camp;   // point-major order; the camera of every point-major position
    int32_t *off_c, *obs_c, *pt_c;   // camera-major order: first position per camera, observation and point per position
    double *V, *gp, *Vi;             // per point: V_p (upper 6), g_p, V_p*^-1 (upper 6)
    double *U, *gc;                  // per camera: U_c (upper 21), g_c
    double *dc, *tpose, *tpts;       // the trial step: camera steps, poses and points
    double* part;                    // per point block: trial cost | |dX|^2 | |X|^2
    sfmloss::Loss loss;              // read by the kRobust kernels only
    double* sw;                      // sqrt(w) per point-major position, for kernels without a residual (else nullptr)
    Calib* cal;                      // the kCal kernels only (else nullptr), with
    double *Wq, *Ucq;                //   W_qp (3 x 3) per point, U_cq (6 x 3) per camera, and per point block
    double* qpart;                   //   U_qq (upper 6) | g_q | sum W_qp V_p*^-1 W_qp^T (upper 6) | sum W_qp V_p*^-1 g_p
};

using sfmhost::Carver;   // csrc/sfm_common.h

// The core's arrays and both orders' buffers (csrc/sfm_obs_order.h), in one fixed sequence.
struct Core {
    Lm lm;
    sfmorder::PointOrder po;
    sfmorder::CameraOrder co;
};

inline Core carve_core(Carver& k, int64_t C, int64_t P, int64_t M, int64_t F, State* st) {
    Core c;
    Lm& w = c.lm;
    w.st = st;
    w.slot = k.take<int32_t>(C);
    w.freec = k.take<int32_t>(F);
    w.off_p = k.take<int32_t>(P + 1);
    int32_t* fill = k.take<int32_t>(P);
    w.ord_p = k.take<int32_t>(M);
    c.po = sfmorder::PointOrder{w.off_p, fill, w.ord_p, k.take<int32_t>(sfmorder::tiles(P)), &st->bad};
    w.camp = k.take<int32_t>(M);
    int32_t* seq0 = k.take<int32_t>(M);
    int32_t* seq1 = k.take<int32_t>(M);
    int32_t* table = k.take<int32_t>(sfmorder::table_size(M));
    int32_t* table_sum = k.take<int32_t>(sfmorder::tiles(sfmorder::table_size(M)));
    w.off_c = k.take<int32_t>(C + 1);
    w.obs_c = k.take<int32_t>(M);
    w.pt_c = k.take<int32_t>(M);
    c.co = sfmorder::CameraOrder{w.camp, seq0, seq1, table, table_sum, w.off_c, w.obs_c, w.pt_c};
    w.V = k.take<double>(6 * P);
    w.gp = k.take<double>(3 * P);
    w.Vi = k.take<double>(6 * P);
    w.U = k.take<double>(21 * C);
    w.gc = k.take<double>(6 * C);
    w.dc = k.take<double>(6 * C);
    w.tpose = k.take<double>(12 * C);
    w.tpts = k.take<double>(3 * P);
    w.part = k.take<double>(3 * ((P + kThreads - 1) / kThreads));
    w.loss = sfmloss::Loss{SFM_BUNDLE_LOSS_SQUARED, 0, 1.0, 1.0};
    w.sw = nullptr;
    w.cal = nullptr;
    w.Wq = w.Ucq = w.qpart = nullptr;
    return c;
}

// Enqueue both orders (off_p zeroed and the state initialised before, on the same stream).  Returns the sequence that
// holds the point-major position of every camera-major position.
inline const int32_t* launch_orders(const Obs& obs, int64_t M, int64_t C, int64_t P, const Core& c, hipStream_t st) {
    sfmorder::launch_point_order(obs.cam, obs.pt, M, C, P, c.po, st);
    return sfmorder::launch_camera_order(obs.cam, obs.pt, M, C, c.po, c.co, st);
}

SFM_DEVICE int upper6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }   // r <= c, 21 entries
SFM_DEVICE int upper3(int r, int c) { return r * 3 - r * (r - 1) / 2 + (c - r); }   // r <= c, 6 entries

SFM_DEVICE void sym3(const double* u, double (&A)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) A[i][j] = A[j][i] = u[upper3(i, j)];
}

SFM_DEVICE void init_state(State* st) {
    State s{};
    s.lambda = kLambda0;
    s.need_lin = 1;
    *st = s;
}

// Sums of the per-block partials in a fixed order (strided per thread, then block_sum over kBlock threads).
template <int K, int kBlock>
SFM_DEVICE void sum_partials(const double* part, int blocks, double* scratch, double* total) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kBlock)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += part[3 * (int64_t)i + k];
    sfm::block_sum<K, kBlock>(v, scratch, total);
}

// The end of a solve, by every thread of a kBlock workgroup: the camera steps dc (x by slot; 0 for a fixed camera and
// for a rejected step, ok = false), the trial poses, the free cameras' share of |delta|^2 and |x|^2, step_ok.
template <int kBlock>
SFM_DEVICE void finish_step(bool ok, const double* x, int C, const double* __restrict__ poses, const Lm& w) {
    __shared__ double part[kBlock / kWave * 2];
    __shared__ double total[2];
    double v[2] = {0.0, 0.0};   // |dc|^2 | |t|^2
    for (int c = threadIdx.x; c < C; c += kBlock) {
        const int s = w.slot[c];
        const double* pose = poses + 12 * (int64_t)c;
        double* out = w.tpose + 12 * (int64_t)c;
        double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (s < 0 || !ok) {
#pragma unroll
            for (int i = 0; i < 12; ++i) out[i] = pose[i];
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = x[6 * (int64_t)s + i];
            sfmpnp::apply_step(pose, d, out);
#pragma unroll
            for (int i = 0; i < 6; ++i) v[0] += d[i] * d[i];
#pragma unroll
            for (int i = 9; i < 12; ++i) v[1] += pose[i] * pose[i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) w.dc[6 * (int64_t)c + i] = d[i];
    }
    sfm::block_sum<2, kBlock>(v, part, total);
    if (threadIdx.x != 0) return;
    w.st->step_ok = ok;
    w.st->dn_c = total[0];
    w.st->xn_c = total[1];
}

// Thread t of a block per free camera takes a contiguous chunk [i0, i1) of camera c's camera-major list.
struct Chunk {
    int c, i0, i1;
};

SFM_DEVICE Chunk camera_chunk(const Lm& w) {
    const int c = w.freec[blockIdx.x];
    const int lo = w.off_c[c], n = w.off_c[c + 1] - lo;
    const int chunk = (n + kThreads - 1) / kThreads;
    return Chunk{c, lo + min(n, (int)threadIdx.x * chunk), lo + min(n, ((int)threadIdx.x + 1) * chunk)};
}

// Jq = dw / d(f, cx, cy) of an observation in front of its camera, times s, from its unweighted residual r = w - (u, v):
// rows ((w_0 - k02) / k00, 1, 0) and ((w_1 - k12) / k00, 0, 1); the column of a held intrinsic is zero.
SFM_DEVICE void intrinsic_rows(const PnPCamera& k, int refine, const double (&r)[2], double u, double v, double s,
                               double (&Jq)[2][3]) {
    const bool focal = refine & SFM_BUNDLE_REFINE_FOCAL, centre = refine & SFM_BUNDLE_REFINE_PRINCIPAL_POINT;
    Jq[0][0] = focal ? s * (((r[0] + u) - k.k02) / k.k00) : 0.0;
    Jq[1][0] = focal ? s * (((r[1] + v) - k.k12) / k.k00) : 0.0;
    Jq[0][1] = Jq[1][2] = centre ? s : 0.0;
    Jq[0][2] = Jq[1][1] = 0.0;
}

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// Linearisation.
// ------------------------------------------------------------------------------------------------------------------------
// Thread per point: the cost of its observations (partial per block; the start needs it), V_p and g_p.  kStoreW (the
// dense path, C <= kLdsCameras): the poses staged in LDS, and W = Jc^T Jp to W[18 q] for every point-major position q of a
// moving point seen by a free camera.  kRobust: the cost is the sum of rho, r, Jc and Jp carry sqrt(w), which also goes to
// w.sw[q] when the adjuster keeps it (0 for an observation behind its camera).  kCal: W_qp of a moving point over all its
// observations, and the block's U_qq and g_q over every observation in front of its camera (held points included).
template <bool kStoreW, bool kRobust, bool kCal = false>
__global__ __launch_bounds__(kThreads) void linearize_kernel(Obs obs, int P, PnPCamera cam, const double* __restrict__ poses,
                                                             const double* __restrict__ points, int C, Lm w,
                                                             double* __restrict__ W) {
    __shared__ double lds_pose[kStoreW ? kLdsCameras * 12 : 1];
    __shared__ double part[kThreads / kWave];
    __shared__ double total[1];
    __shared__ double qpart[kCal ? kThreads / kWave * 9 : 1];
    __shared__ double qtotal[kCal ? 9 : 1];
    if (w.st->stop || w.st->bad || !w.st->need_lin) return;
    if (kCal) cam = w.cal->cam;
    const double* pose = poses;
    if (kStoreW) {
        for (int k = threadIdx.x; k < 12 * C; k += kThreads) lds_pose[k] = poses[k];
        __syncthreads();
        pose = lds_pose;
    }
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double e[1] = {0.0};
    double qs[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // kCal: U_qq (upper 6) | g_q
    if (p < P) {
        const double X = points[3 * (int64_t)p], Y = points[3 * (int64_t)p + 1], Z = points[3 * (int64_t)p + 2];
        const int q0 = w.off_p[p], q1 = w.off_p[p + 1];
        const bool moving = q1 - q0 >= 2;
        double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        double Wq[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int q = q0; q < q1; ++q) {
            const int m = w.ord_p[q];
            const int c = w.camp[q];
            const double* mp = pose + 12 * (int64_t)c;
            const double u = obs.uv[2 * (int64_t)m], v = obs.uv[2 * (int64_t)m + 1];
            const double eq = sfmpnp::pnp_score(mp, cam, X, Y, Z, u, v);
            e[0] += kRobust ? sfmloss::rho(w.loss, eq) : eq;
            double r[2], Jc[2][6], Jp[2][3];
            const bool front = sfmpnp::jacobians(mp, cam, X, Y, Z, Jc, Jp, r, u, v);
            double s = 1.0;
            if (kRobust) {
                s = front ? sfmloss::sqrt_weight(w.loss, r) : 0.0;
                if (w.sw) w.sw[q] = s;
            }
            if (!front) continue;
            double Jq[2][3];
            if (kCal) intrinsic_rows(cam, w.cal->refine, r, u, v, s, Jq);
            if (kRobust) sfmloss::scale(s, r, Jc, Jp);
            if (kCal) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = i; j < 3; ++j) qs[upper3(i, j)] += Jq[0][i] * Jq[0][j] + Jq[1][i] * Jq[1][j];
                    qs[6 + i] += Jq[0][i] * r[0] + Jq[1][i] * r[1];
                    if (moving) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) Wq[3 * i + j] += Jq[0][i] * Jp[0][j] + Jq[1][i] * Jp[1][j];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = i; j < 3; ++j) V[upper3(i, j)] += Jp[0][i] * Jp[0][j] + Jp[1][i] * Jp[1][j];
                g[i] += Jp[0][i] * r[0] + Jp[1][i] * r[1];
            }
            if (kStoreW && moving && w.slot[c] >= 0) {
                double* Wq = W + 18 * (int64_t)q;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) Wq[3 * i + j] = Jc[0][i] * Jp[0][j] + Jc[1][i] * Jp[1][j];
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) w.V[6 * (int64_t)p + k] = V[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) w.gp[3 * (int64_t)p + k] = g[k];
        if (kCal) {
#pragma unroll
            for (int k = 0; k < 9; ++k) w.Wq[9 * (int64_t)p + k] = Wq[k];
        }
    }
    sfm::block_sum<1, kThreads>(e, part, total);
    if (threadIdx.x == 0) w.part[3 * (int64_t)blockIdx.x] = total[0];
    if (kCal) {
        sfm::block_sum<9, kThreads>(qs, qpart, qtotal);
        if (threadIdx.x < 9) w.qpart[18 * (int64_t)blockIdx.x + threadIdx.x] = qtotal[threadIdx.x];
    }
}

// Block per free camera: U_c (upper 21) and g_c over its observations in camera-major order.  kRobust: sqrt(w) again
// from the residual, the bits linearize_kernel got.  kCal: U_cq (6 x 3) as well.
template <bool kRobust, bool kCal = false>
__global__ __launch_bounds__(kThreads) void camera_kernel(Obs obs, PnPCamera cam, const double* __restrict__ poses,
                                                          const double* __restrict__ points, Lm w) {
    constexpr int kSums = kCal ? 45 : 27;
    __shared__ double part[kThreads / kWave * kSums];
    __shared__ double total[kSums];
    if (w.st->stop || w.st->bad || !w.st->need_lin) return;
    if (kCal) cam = w.cal->cam;
    const Chunk ch = camera_chunk(w);
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * (int64_t)ch.c + k];
    double a[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) a[k] = 0.0;
    for (int i = ch.i0; i < ch.i1; ++i) {
        const int64_t mo = w.obs_c[i], p = w.pt_c[i];
        double r[2], Jc[2][6], Jp[2][3];
        if (!sfmpnp::jacobians(m, cam, points[3 * p], points[3 * p + 1], points[3 * p + 2], Jc, Jp, r, obs.uv[2 * mo],
                               obs.uv[2 * mo + 1]))
            continue;
        const double s = kRobust ? sfmloss::sqrt_weight(w.loss, r) : 1.0;
        double Jq[2][3];
        if (kCal) intrinsic_rows(cam, w.cal->refine, r, obs.uv[2 * mo], obs.uv[2 * mo + 1], s, Jq);
        if (kRobust) sfmloss::scale(s, r, Jc, Jp);
#pragma unroll
        for (int x = 0; x < 6; ++x) {
#pragma unroll
            for (int y = x; y < 6; ++y) a[upper6(x, y)] += Jc[0][x] * Jc[0][y] + Jc[1][x] * Jc[1][y];
            a[21 + x] += Jc[0][x] * r[0] + Jc[1][x] * r[1];
            if (kCal) {
#pragma unroll
                for (int y = 0; y < 3; ++y) a[27 + 3 * x + y] += Jc[0][x] * Jq[0][y] + Jc[1][x] * Jq[1][y];
            }
        }
    }
    sfm::block_sum<kSums, kThreads>(a, part, total);
    if (threadIdx.x < 21) w.U[21 * (int64_t)ch.c + threadIdx.x] = total[threadIdx.x];
    else if (threadIdx.x < 27) w.gc[6 * (int64_t)ch.c + threadIdx.x - 21] = total[threadIdx.x];
    else if (kCal && threadIdx.x < 45) w.Ucq[18 * (int64_t)ch.c + threadIdx.x - 27] = total[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------------
// One LM trial step: the damped point blocks before the solve; the decision and the commit after the trial.
// ------------------------------------------------------------------------------------------------------------------------
// Thread per moving point: V_p* = V_p + lambda diag V_p, its 3 x 3 Cholesky (sfm_lm.h), and V_p*^-1 (upper 6).  A pivot
// <= 0 or not finite marks the step as failed.
__global__ __launch_bounds__(kThreads) void point_kernel(int P, Lm w) {
    if (w.st->stop) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P || w.off_p[p + 1] - w.off_p[p] < 2) return;
    const double lambda = w.st->lambda;
    double A[3][3];
    sym3(w.V + 6 * (int64_t)p, A);
#pragma unroll
    for (int i = 0; i < 3; ++i) A[i][i] = A[i][i] + lambda * A[i][i];
    double L[3][3], inv[3][3];
    if (!factor<3>(A, 0.0, L)) {
        w.st->fail = 1;
        return;
    }
    inverse<3>(L, inv);
    double* out = w.Vi + 6 * (int64_t)p;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) out[upper3(i, j)] = inv[i][j];
}

// After the first linearisation: an index out of range stops the call; else the starting cost, the bad-start status and
// the gauge (fixed camera f, anchor a).
template <int kBlock>
__global__ __launch_bounds__(kBlock) void start_kernel(int blocks, int f, int a, int max_steps,
                                                       const double* __restrict__ poses, Lm w) {
    __shared__ double scratch[kBlock / kWave * 3];
    __shared__ double total[3];
    State* st = w.st;
    if (st->bad) {
        if (threadIdx.x == 0) {
            st->status = SFM_BUNDLE_BAD_INDEX;
            st->stop = 1;
        }
        return;
    }
    sum_partials<1, kBlock>(w.part, blocks, scratch, total);
    if (threadIdx.x != 0) return;
    const double c = total[0];
    st->initial_cost = st->cost = c;
    if (!isfinite(c)) {
        st->status = SFM_BUNDLE_BAD_START;
        st->stop = 1;
        return;
    }
    st->stop = max_steps <= 0;
    st->need_lin = 0;   // the launches before this one linearised the start
    if (a >= 0) {
        double c0[3], ca[3];
        sfmpnp::centre(poses + 12 * (int64_t)f, c0);
        sfmpnp::centre(poses + 12 * (int64_t)a, ca);
        const double d0 = ca[0] - c0[0], d1 = ca[1] - c0[1], d2 = ca[2] - c0[2];
        st->dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        for (int k = 0; k < 3; ++k) st->c0[k] = c0[k];
    }
}

// Accept or reject the trial: the cost in a fixed order, lambda, the gauge scale (anchor a), the stops.
template <int kBlock>
__global__ __launch_bounds__(kBlock) void decide_kernel(int blocks, int a, int max_steps, Lm w) {
    __shared__ double scratch[kBlock / kWave * 3];
    __shared__ double total[3];
    State* st = w.st;
    const bool stop = st->stop, step_ok = st->step_ok;
    __syncthreads();   // every thread has read the state before thread 0 writes it
    if (threadIdx.x == 0) st->commit = 0;
    if (stop) return;
    if (step_ok) sum_partials<3, kBlock>(w.part, blocks, scratch, total);   // block-uniform
    if (threadIdx.x != 0) return;
    st->steps += 1;
    st->fail = 0;
    double lambda = st->lambda;
    bool done = false;
    if (!step_ok) {
        lambda = more_damping(lambda);
    } else {
        const double dn = total[1] + st->dn_c, xn = total[2] + st->xn_c;
        const double c_new = total[0], c_old = st->cost;
        if (small_step(sqrt(dn), sqrt(xn))) {   // here and not before the trial: the points' share is known only now
            done = true;
        } else if (improved(c_new, c_old)) {
            done = converged(c_old, c_new);
            st->cost = c_new;
            st->accepted += 1;
            st->commit = 1;
            st->need_lin = 1;
            lambda = less_damping(lambda);
            if (a >= 0) {
                double ca[3];
                sfmpnp::centre(w.tpose + 12 * (int64_t)a, ca);
                const double d0 = ca[0] - st->c0[0], d1 = ca[1] - st->c0[1], d2 = ca[2] - st->c0[2];
                st->scale = st->dist / sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            }
        } else {
            lambda = more_damping(lambda);
        }
    }
    st->lambda = lambda;
    st->stop = done || exhausted(st->steps, max_steps, lambda);
}

// An accepted trial becomes the current estimate; with one fixed camera (a >= 0), scaled about its centre by st->scale.
// Thread i takes point i and camera i.  kCal: the trial camera becomes the current one, untouched by the rescale.
template <bool kCal = false>
__global__ __launch_bounds__(kThreads) void commit_kernel(int P, int C, int a, double* __restrict__ poses,
                                                          double* __restrict__ points, Lm w) {
    const State* st = w.st;
    if (!st->commit) return;
    if (kCal && blockIdx.x == 0 && threadIdx.x == 0) w.cal->cam = w.cal->trial;
    const bool rescale = a >= 0;
    const double s = st->scale, c0[3] = {st->c0[0], st->c0[1], st->c0[2]};
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < P) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = w.tpts[3 * (int64_t)i + k];
            points[3 * (int64_t)i + k] = rescale ? c0[k] + s * (x - c0[k]) : x;
        }
    }
    if (i < C && w.slot[i] >= 0) {
        const double* tp = w.tpose + 12 * (int64_t)i;
        double* out = poses + 12 * (int64_t)i;
        for (int k = 0; k < 9; ++k) out[k] = tp[k];
        if (rescale) {
            double cc[3];
            sfmpnp::centre(tp, cc);
            for (int k = 0; k < 3; ++k) cc[k] = c0[k] + s * (cc[k] - c0[k]);
            for (int r = 0; r < 3; ++r) out[9 + r] = -((tp[3 * r] * cc[0] + tp[3 * r + 1] * cc[1]) + tp[3 * r + 2] * cc[2]);
        } else {
            for (int r = 0; r < 3; ++r) out[9 + r] = tp[9 + r];
        }
    }
}

}  // namespace

// The fields both info records share (sfm_bundle_info, sfm_bundle_pcg_info), reserved = 0.
template <class Info>
SFM_DEVICE void write_info(const State* st, Info* info) {
    const bool bad_index = st->status == SFM_BUNDLE_BAD_INDEX;
    info->initial_cost = bad_index ? NAN : st->initial_cost;
    info->final_cost = bad_index ? NAN : st->cost;
    info->steps = st->steps;
    info->accepted = st->accepted;
    info->status = st->status;
    info->reserved = 0;
}

}  // namespace sfmlm
