// Bundle adjustment with an iterative Schur solver: the Levenberg-Marquardt loop of sfm_bundle.hip over
// any number of cameras, with the damped reduced camera system S* dc = b solved by conjugate gradients preconditioned
// with S*'s 6 x 6 diagonal blocks (block Jacobi).  S* = U* - W V*^-1 W^T is applied matrix-free and never formed
// (the NumPy oracle is tests/bundle_pcg_oracle.py).  fp64 throughout; off unless asked for.
//
// The Jacobians are recomputed from the pose and the point wherever W = Jc^T Jp is needed, instead of storing W (144 B
// per observation): W^T x = Jp^T (Jc x) and W y = Jc^T (Jp y).  A pass then reads the indices, the point and the pose.
//
// Set-up, once per call: the point-major order (csrc/sfm_obs_order.h) and a camera-major order by a stable LSD radix
// sort of the point-major positions on the camera index, 8 bits per pass (per-tile digit counts: 256 words per 1 024
// observations, whatever the camera count), so that inside a camera the observations are sorted by point.  No order
// depends on the order atomics ran in.  Then per LM trial step, every launch reading the LM state first and returning at
// once after a stop:
//   pcg_linearize_kernel   (after an accepted step)  thread per point: V_p, g_p and the cost of its observations
//   pcg_camera_kernel      (after an accepted step)  block per free camera: U_c and g_c over its camera-major list
//   pcg_point_kernel       thread per point: V_p* = V_p + lambda diag V_p and its inverse
//   pcg_precond_kernel     block per free camera: M_c = U*_c - sum_p W_cp V_p*^-1 W_cp^T, b_c, and M_c^-1 by Cholesky
//   pcg_cg_init_kernel     one workgroup: x = 0, r = b, z = M^-1 r, p = z
//   per CG iteration:      pcg_cg_point_kernel  (thread per point: y_p = V_p*^-1 sum W^T p_c)
//                          pcg_cg_camera_kernel (block per free camera: q_c = U*_c p_c - sum W y_p, and p_c . q_c)
//                          pcg_cg_update_kernel (one workgroup: alpha, x, r, z, rho, beta, p and the stop of CG)
//   pcg_apply_kernel       one workgroup: the camera steps, the trial poses and the camera part of |delta|, |x|
//   pcg_trial_kernel       thread per point: back-substitution dX_p, the trial point, its observations' trial cost
//   pcg_decide_kernel      one workgroup: accept / reject, lambda, the gauge scale, stops (the dense path's rules)
//   pcg_commit_kernel      an accepted trial becomes the current estimate (rescaled when one camera is fixed)
// The host reads two flags (LM stop, CG done) from pinned memory once per LM step and once per chunk of kCgChunk CG
// iterations, and enqueues no more work after a stop.  The device state alone decides the result: every kernel also
// returns at once after a stop, so the reads only save launches.  No floating-point atomics anywhere: every sum runs in
// an order fixed by the sizes alone, so a call is bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_obs_order.h"
#include "sfm_pnp.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmpnp::camera_from;
using sfmpnp::pnp_score;
using sfmpnp::PnPCamera;

constexpr int kThreads = 256;         // point-parallel and per-camera kernels
constexpr int kOneGroup = 1024;       // the one-workgroup kernels
constexpr int kRadixTile = 1024;      // observations per workgroup of a radix pass
constexpr int kRadixBits = 8;
constexpr int kDigits = 1 << kRadixBits;
constexpr int kCgChunk = 10;          // CG iterations enqueued between two reads of the flags
constexpr double kLambda0 = 1e-3;
constexpr double kLambdaMax = 1e16;
constexpr double kMinDecrease = 1e-12;
constexpr double kMinStep = 1e-12;

static_assert(sizeof(sfm_bundle_pcg_info) == 40, "sfm_bundle_pcg_info layout is part of the ABI");

// The LM and CG state: written by one thread of the one-workgroup kernels, read by every launch after it.
struct State {
    double lambda, cost, initial_cost, scale;
    double c0[3], dist;     // gauge: the fixed camera's centre and the anchor camera's distance from it
    double rho, tol2;       // CG: r^T z, and tol^2 |b|^2
    double dn_c, xn_c;      // the free cameras' share of |delta|^2 and |x|^2 of this trial step
    int32_t stop, cg_done;  // adjacent: the host reads both at once
    int32_t steps, accepted, status;
    int32_t need_lin;       // the current estimate has no linearisation yet (start, or an accepted step)
    int32_t step_ok;        // the step is finite and CG did not fail
    int32_t commit;         // this step's trial was accepted
    int32_t fail;           // a V_p* or an M_c did not factor (any thread may set it)
    int32_t cg_fail;        // this step is rejected (a failed factorisation or a breakdown at k = 0)
    int32_t cg_k, cg_total, cg_max;
    int32_t bad;            // an index is out of range (set by the point order's count kernel)
    int32_t pad[2];
};

struct Layout {
    size_t state, slot, freec, off_p, fill_p, ord_p, tsum_p, camp, seq0, seq1, table, tsum_r, off_c, pt_c, obs_c, V, gp, Vi,
        y, U, gc, Minv, b, x, r, z, p, q, part, dc, tpose, tpts, ppart, total;
};

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

int64_t radix_tiles(int64_t M) { return (M + kRadixTile - 1) / kRadixTile; }

Layout layout(int64_t C, int64_t P, int64_t M, int64_t F) {
    Layout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o = align256(o + (bytes > 0 ? bytes : 8));
        return (size_t)at;
    };
    const int64_t table = kDigits * radix_tiles(M) + 1;
    const int64_t pblocks = (P + kThreads - 1) / kThreads;
    L.state = take(sizeof(State));
    L.slot = take(4 * C);
    L.freec = take(4 * F);
    L.off_p = take(4 * (P + 1));
    L.fill_p = take(4 * P);
    L.ord_p = take(4 * M);
    L.tsum_p = take(4 * sfmorder::tiles(P));
    L.camp = take(4 * M);
    L.seq0 = take(4 * M);
    L.seq1 = take(4 * M);
    L.table = take(4 * table);
    L.tsum_r = take(4 * sfmorder::tiles(table));
    L.off_c = take(4 * (C + 1));
    L.pt_c = take(4 * M);
    L.obs_c = take(4 * M);
    L.V = take(8 * 6 * P);
    L.gp = take(8 * 3 * P);
    L.Vi = take(8 * 6 * P);
    L.y = take(8 * 3 * P);
    L.U = take(8 * 21 * C);
    L.gc = take(8 * 6 * C);
    L.Minv = take(8 * 36 * F);
    L.b = take(8 * 6 * F);
    L.x = take(8 * 6 * F);
    L.r = take(8 * 6 * F);
    L.z = take(8 * 6 * F);
    L.p = take(8 * 6 * F);
    L.q = take(8 * 6 * F);
    L.part = take(8 * F);
    L.dc = take(8 * 6 * C);
    L.tpose = take(8 * 12 * C);
    L.tpts = take(8 * 3 * P);
    L.ppart = take(8 * 3 * (pblocks > 0 ? pblocks : 1));
    L.total = (size_t)o;
    return L;
}

struct Ws {
    State* st;
    int32_t *slot, *freec, *off_p, *fill_p, *ord_p, *tsum_p, *camp, *seq0, *seq1, *table, *tsum_r, *off_c, *pt_c, *obs_c;
    double *V, *gp, *Vi, *y, *U, *gc, *Minv, *b, *x, *r, *z, *p, *q, *part, *dc, *tpose, *tpts, *ppart;
};

Ws carve(void* base, const Layout& L) {
    char* c = static_cast<char*>(base);
    auto i32 = [&](size_t at) { return reinterpret_cast<int32_t*>(c + at); };
    auto f64 = [&](size_t at) { return reinterpret_cast<double*>(c + at); };
    Ws w;
    w.st = reinterpret_cast<State*>(c + L.state);
    w.slot = i32(L.slot);
    w.freec = i32(L.freec);
    w.off_p = i32(L.off_p);
    w.fill_p = i32(L.fill_p);
    w.ord_p = i32(L.ord_p);
    w.tsum_p = i32(L.tsum_p);
    w.camp = i32(L.camp);
    w.seq0 = i32(L.seq0);
    w.seq1 = i32(L.seq1);
    w.table = i32(L.table);
    w.tsum_r = i32(L.tsum_r);
    w.off_c = i32(L.off_c);
    w.pt_c = i32(L.pt_c);
    w.obs_c = i32(L.obs_c);
    w.V = f64(L.V);
    w.gp = f64(L.gp);
    w.Vi = f64(L.Vi);
    w.y = f64(L.y);
    w.U = f64(L.U);
    w.gc = f64(L.gc);
    w.Minv = f64(L.Minv);
    w.b = f64(L.b);
    w.x = f64(L.x);
    w.r = f64(L.r);
    w.z = f64(L.z);
    w.p = f64(L.p);
    w.q = f64(L.q);
    w.part = f64(L.part);
    w.dc = f64(L.dc);
    w.tpose = f64(L.tpose);
    w.tpts = f64(L.tpts);
    w.ppart = f64(L.ppart);
    return w;
}

struct Obs {
    const int32_t* cam;
    const int32_t* pt;
    const double* uv;
};

// Block-wide sums of K doubles per thread in a fixed order: butterfly inside each wave, then the wave partials added in
// wave order.  Valid in `total` for every thread after the call.
template <int K, int kBlock>
SFM_DEVICE void block_sum(double (&v)[K], double (*part)[K], double* total) {
    constexpr int kWaves = kBlock / kWave;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = sfm::wave_sum(v[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += kBlock) {
        double acc = part[0][k];
        for (int w = 1; w < kWaves; ++w) acc += part[w][k];
        total[k] = acc;
    }
    __syncthreads();
}

// The Jacobian rows of one observation in front of the camera, as sfm_bundle.hip's linearize (row k of Jc =
// (R X x A_k, A_k), of Jp = A_k R); with the residual when r is given.  False behind the camera.
SFM_DEVICE bool jacobians(const double* m, const PnPCamera& k, double X, double Y, double Z, double (&Jc)[2][6],
                          double (&Jp)[2][3], double* r = nullptr, double u = 0.0, double v = 0.0) {
    const double r0 = (m[0] * X + m[1] * Y) + m[2] * Z;
    const double r1 = (m[3] * X + m[4] * Y) + m[5] * Z;
    const double r2 = (m[6] * X + m[7] * Y) + m[8] * Z;
    const double c0 = r0 + m[9], c1 = r1 + m[10], c2 = r2 + m[11];
    if (!(c2 > 0.0)) return false;
    const double w0 = ((k.k00 * c0 + k.k01 * c1) + k.k02 * c2) / c2;
    const double w1 = ((k.k10 * c0 + k.k11 * c1) + k.k12 * c2) / c2;
    if (r) {
        r[0] = w0 - u;
        r[1] = w1 - v;
    }
    const double ic = 1.0 / c2;
    const double A[2][3] = {{k.k00 * ic, k.k01 * ic, (k.k02 - w0) * ic}, {k.k10 * ic, k.k11 * ic, (k.k12 - w1) * ic}};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        Jc[q][0] = r1 * A[q][2] - r2 * A[q][1];
        Jc[q][1] = r2 * A[q][0] - r0 * A[q][2];
        Jc[q][2] = r0 * A[q][1] - r1 * A[q][0];
        Jc[q][3] = A[q][0];
        Jc[q][4] = A[q][1];
        Jc[q][5] = A[q][2];
#pragma unroll
        for (int j = 0; j < 3; ++j) Jp[q][j] = (A[q][0] * m[j] + A[q][1] * m[3 + j]) + A[q][2] * m[6 + j];
    }
    return true;
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

SFM_DEVICE int upper6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }   // r <= c, 21 entries
SFM_DEVICE int upper3(int r, int c) { return r * 3 - r * (r - 1) / 2 + (c - r); }   // r <= c, 6 entries

SFM_DEVICE void sym3(const double* u, double (&A)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) A[i][j] = A[j][i] = u[upper3(i, j)];
}

// out = {exp([w]x) R | t + dt}: Rodrigues with the Taylor forms below th = 1e-6 (sfm_bundle.hip's apply_step)
SFM_DEVICE void apply_step(const double* pose, const double* delta, double* out) {
    const double w0 = delta[0], w1 = delta[1], w2 = delta[2];
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    const double th = sqrt(th2);
    double A, B;
    if (th < 1e-6) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
    } else {
        const double s = sin(0.5 * th);
        A = sin(th) / th;
        B = 2.0 * s * s / th2;
    }
    const double W[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double E[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double W2 = (W[r][0] * W[0][c] + W[r][1] * W[1][c]) + W[r][2] * W[2][c];
            E[r][c] = ((r == c ? 1.0 : 0.0) + A * W[r][c]) + B * W2;
        }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (E[r][0] * pose[c] + E[r][1] * pose[3 + c]) + E[r][2] * pose[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[9 + r] = pose[9 + r] + delta[3 + r];
}

SFM_DEVICE void centre(const double* pose, double (&c)[3]) {   // -R^T t
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = -((pose[k] * pose[9] + pose[3 + k] * pose[10]) + pose[6 + k] * pose[11]);
}

// ------------------------------------------------------------------------------------------------------------------------
// Set-up.
// ------------------------------------------------------------------------------------------------------------------------
// The state; the free cameras' list from the slots (slot[c] = -1 for a fixed camera)
__global__ __launch_bounds__(kThreads) void pcg_init_kernel(int C, Ws w) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c == 0) {
        State s{};
        s.lambda = kLambda0;
        s.need_lin = 1;
        *w.st = s;
    }
    if (c < C && w.slot[c] >= 0) w.freec[w.slot[c]] = c;
}

// After the point order: an index out of range stops the call; else the camera of every point-major position and the
// identity sequence the radix passes sort
__global__ __launch_bounds__(kThreads) void pcg_positions_kernel(Obs obs, int M, Ws w) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (w.st->bad) {
        if (q == 0) {
            w.st->status = SFM_BUNDLE_BAD_INDEX;
            w.st->stop = 1;
        }
        return;
    }
    if (q >= M) return;
    w.camp[q] = obs.cam[w.ord_p[q]];
    w.seq0[q] = q;
}

// One stable LSD radix pass over the sequence src of point-major positions, keyed by the digit of their camera at
// `shift`.  kScatter = false: the tile's count of every digit to table[digit * tiles + tile].  kScatter = true (after the
// exclusive scan of the table): every position to its place in dst.  Rank inside a tile: the lanes of a wave with the same
// digit by 8 ballots, then the waves in order.
template <bool kScatter>
__global__ __launch_bounds__(kRadixTile) void pcg_radix_kernel(int M, int shift, int tiles, const int32_t* __restrict__ src,
                                                               int32_t* __restrict__ dst, Ws w) {
    constexpr int kWaves = kRadixTile / kWave;
    __shared__ int32_t wcount[kWaves][kDigits];
    if (w.st->bad) return;
    for (int k = threadIdx.x; k < kWaves * kDigits; k += kRadixTile) (&wcount[0][0])[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = blockIdx.x * kRadixTile + threadIdx.x;
    const bool valid = i < M;
    const int32_t q = valid ? src[i] : 0;
    const int d = valid ? (w.camp[q] >> shift) & (kDigits - 1) : 0;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < kRadixBits; ++bit) {
        const bool set = (d >> bit) & 1;
        const uint64_t b = __ballot(set);
        peers &= set ? b : ~b;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcount[wave][d] = __popcll(peers);
    __syncthreads();
    if (!kScatter) {
        for (int k = threadIdx.x; k < kDigits; k += kRadixTile) {
            int32_t n = 0;
            for (int v = 0; v < kWaves; ++v) n += wcount[v][k];
            w.table[(int64_t)k * tiles + blockIdx.x] = n;
        }
    } else if (valid) {
        int32_t before = 0;
        for (int v = 0; v < wave; ++v) before += wcount[v][d];
        dst[w.table[(int64_t)d * tiles + blockIdx.x] + before + rank] = q;
    }
}

// After the last pass: camera-major position i -> observation and point; off_c[c] = first position of camera c
__global__ __launch_bounds__(kThreads) void pcg_camera_order_kernel(Obs obs, int M, int C, const int32_t* __restrict__ seq,
                                                                    Ws w) {
    if (w.st->bad) return;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i > M) return;
    const int key = i < M ? w.camp[seq[i]] : C;
    const int prev = i > 0 ? w.camp[seq[i - 1]] : -1;
    for (int c = prev + 1; c <= key; ++c) w.off_c[c] = i;
    if (i < M) {
        const int32_t m = w.ord_p[seq[i]];
        w.obs_c[i] = m;
        w.pt_c[i] = obs.pt[m];
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Linearisation.
// ------------------------------------------------------------------------------------------------------------------------
// Thread per point: the cost of its observations (partial per block; the start needs it), V_p and g_p.
__global__ __launch_bounds__(kThreads) void pcg_linearize_kernel(Obs obs, int P, PnPCamera cam,
                                                                 const double* __restrict__ poses,
                                                                 const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave][1];
    __shared__ double total[1];
    if (w.st->stop || !w.st->need_lin) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double e[1] = {0.0};
    if (p < P) {
        const double X = points[3 * (int64_t)p], Y = points[3 * (int64_t)p + 1], Z = points[3 * (int64_t)p + 2];
        const int q0 = w.off_p[p], q1 = w.off_p[p + 1];
        double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        for (int q = q0; q < q1; ++q) {
            const int m = w.ord_p[q];
            const double* mp = poses + 12 * (int64_t)w.camp[q];
            const double u = obs.uv[2 * (int64_t)m], v = obs.uv[2 * (int64_t)m + 1];
            e[0] += pnp_score(mp, cam, X, Y, Z, u, v);
            double r[2], Jc[2][6], Jp[2][3];
            if (!jacobians(mp, cam, X, Y, Z, Jc, Jp, r, u, v)) continue;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = i; j < 3; ++j) V[upper3(i, j)] += Jp[0][i] * Jp[0][j] + Jp[1][i] * Jp[1][j];
                g[i] += Jp[0][i] * r[0] + Jp[1][i] * r[1];
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) w.V[6 * (int64_t)p + k] = V[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) w.gp[3 * (int64_t)p + k] = g[k];
    }
    block_sum<1, kThreads>(e, part, total);
    if (threadIdx.x == 0) w.ppart[3 * (int64_t)blockIdx.x] = total[0];
}

// Thread t of a per-camera block takes a contiguous chunk of the camera's list.
struct Chunk {
    int c, i0, i1;
};

SFM_DEVICE Chunk camera_chunk(const Ws& w) {
    const int c = w.freec[blockIdx.x];
    const int lo = w.off_c[c], n = w.off_c[c + 1] - lo;
    const int chunk = (n + kThreads - 1) / kThreads;
    return Chunk{c, lo + min(n, (int)threadIdx.x * chunk), lo + min(n, ((int)threadIdx.x + 1) * chunk)};
}

// Block per free camera: U_c (upper 21) and g_c over its observations in camera-major order.
__global__ __launch_bounds__(kThreads) void pcg_camera_kernel(Obs obs, PnPCamera cam, const double* __restrict__ poses,
                                                              const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave][27];
    __shared__ double total[27];
    if (w.st->stop || !w.st->need_lin) return;
    const Chunk ch = camera_chunk(w);
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * (int64_t)ch.c + k];
    double a[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) a[k] = 0.0;
    for (int i = ch.i0; i < ch.i1; ++i) {
        const int64_t mo = w.obs_c[i], p = w.pt_c[i];
        double r[2], Jc[2][6], Jp[2][3];
        if (!jacobians(m, cam, points[3 * p], points[3 * p + 1], points[3 * p + 2], Jc, Jp, r, obs.uv[2 * mo],
                       obs.uv[2 * mo + 1]))
            continue;
#pragma unroll
        for (int x = 0; x < 6; ++x) {
#pragma unroll
            for (int y = x; y < 6; ++y) a[upper6(x, y)] += Jc[0][x] * Jc[0][y] + Jc[1][x] * Jc[1][y];
            a[21 + x] += Jc[0][x] * r[0] + Jc[1][x] * r[1];
        }
    }
    block_sum<27, kThreads>(a, part, total);
    if (threadIdx.x < 21) w.U[21 * (int64_t)ch.c + threadIdx.x] = total[threadIdx.x];
    else if (threadIdx.x < 27) w.gc[6 * (int64_t)ch.c + threadIdx.x - 21] = total[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------------
// One LM trial step: the damped point blocks, the preconditioner and the right-hand side.
// ------------------------------------------------------------------------------------------------------------------------
// Thread per moving point: V_p* = V_p + lambda diag V_p, its 3 x 3 Cholesky, and V_p*^-1 (upper 6).  A pivot <= 0 or not
// finite marks the step as failed.
__global__ __launch_bounds__(kThreads) void pcg_point_kernel(int P, Ws w) {
    if (w.st->stop) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P || w.off_p[p + 1] - w.off_p[p] < 2) return;
    const double lambda = w.st->lambda;
    double A[3][3];
    sym3(w.V + 6 * (int64_t)p, A);
#pragma unroll
    for (int i = 0; i < 3; ++i) A[i][i] = A[i][i] + lambda * A[i][i];
    double L[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        ok = ok && s > 0.0 && isfinite(s);
        L[j][j] = sqrt(fmax(s, 0.0));
#pragma unroll
        for (int i = j + 1; i < 3; ++i) {
            double x = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) x -= L[i][k] * L[j][k];
            L[i][j] = x / L[j][j];
        }
    }
    if (!ok) {
        w.st->fail = 1;
        return;
    }
    double Li[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = c; i < 3; ++i) {
            double x = i == c ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k) x -= L[i][k] * Li[k][c];
            Li[i][c] = x / L[i][i];
        }
    double* out = w.Vi + 6 * (int64_t)p;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) out[upper3(i, j)] = (Li[0][i] * Li[0][j] + Li[1][i] * Li[1][j]) + Li[2][i] * Li[2][j];
}

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
// sum W V_p*^-1 g_p, and M_c^-1 (full 36) from its Cholesky factor.  A pivot <= 0 or not finite marks the step as failed.
__global__ __launch_bounds__(kThreads) void pcg_precond_kernel(PnPCamera cam, const double* __restrict__ poses,
                                                               const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave][27];
    __shared__ double total[27];
    if (w.st->stop || w.st->fail) return;
    const Chunk ch = camera_chunk(w);
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * (int64_t)ch.c + k];
    double a[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) a[k] = 0.0;
    for (int i = ch.i0; i < ch.i1; ++i) {
        const int64_t p = w.pt_c[i];
        if (w.off_p[p + 1] - w.off_p[p] < 2) continue;
        double Jc[2][6], Jp[2][3];
        if (!jacobians(m, cam, points[3 * p], points[3 * p + 1], points[3 * p + 2], Jc, Jp)) continue;
        double Wm[6][3], Vi[3][3], Y[6][3];
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int j = 0; j < 3; ++j) Wm[x][j] = Jc[0][x] * Jp[0][j] + Jc[1][x] * Jp[1][j];
        sym3(w.Vi + 6 * p, Vi);
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int j = 0; j < 3; ++j) Y[x][j] = (Wm[x][0] * Vi[0][j] + Wm[x][1] * Vi[1][j]) + Wm[x][2] * Vi[2][j];
        const double* g = w.gp + 3 * p;
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
    damped_u(w.U + 21 * (int64_t)ch.c, w.st->lambda, A);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = A[i][j] - total[upper6(i, j)];
#pragma unroll
    for (int i = 0; i < 6; ++i) w.b[6 * (int64_t)s + i] = -w.gc[6 * (int64_t)ch.c + i] + total[21 + i];
    double L[6][6] = {};
    bool ok = true;
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0 && isfinite(d);
        L[j][j] = sqrt(fmax(d, 0.0));
        for (int i = j + 1; i < 6; ++i) {
            double x = A[i][j];
            for (int k = 0; k < j; ++k) x -= L[i][k] * L[j][k];
            L[i][j] = x / L[j][j];
        }
    }
    if (!ok) {
        w.st->fail = 1;
        return;
    }
    double Li[6][6] = {};
    for (int c = 0; c < 6; ++c)
        for (int i = c; i < 6; ++i) {
            double x = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) x -= L[i][k] * Li[k][c];
            Li[i][c] = x / L[i][i];
        }
    double* out = w.Minv + 36 * (int64_t)s;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
            for (int k = max(i, j); k < 6; ++k) v += Li[k][i] * Li[k][j];
            out[6 * i + j] = v;
        }
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
// rho or |b|^2 rejects the step.
__global__ __launch_bounds__(kOneGroup) void pcg_cg_init_kernel(int F, double tol, Ws w) {
    __shared__ double part[kOneGroup / kWave][2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->stop) return;
    const bool failed = st->fail;
    __syncthreads();   // every thread has read the state before thread 0 writes it
    if (threadIdx.x == 0) {
        st->need_lin = 0;   // the linearisation kernels of this step have run
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
__global__ __launch_bounds__(kThreads) void pcg_cg_point_kernel(int P, PnPCamera cam, const double* __restrict__ poses,
                                                                const double* __restrict__ points, Ws w) {
    if (w.st->stop || w.st->cg_done) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int q0 = w.off_p[p], q1 = w.off_p[p + 1];
    double t[3] = {0.0, 0.0, 0.0};
    if (q1 - q0 >= 2) {
        const double X = points[3 * (int64_t)p], Y = points[3 * (int64_t)p + 1], Z = points[3 * (int64_t)p + 2];
        for (int q = q0; q < q1; ++q) {
            const int c = w.camp[q], s = w.slot[c];
            if (s < 0) continue;
            double Jc[2][6], Jp[2][3], d[3];
            if (!jacobians(poses + 12 * (int64_t)c, cam, X, Y, Z, Jc, Jp)) continue;
            wt_times(Jc, Jp, w.p + 6 * (int64_t)s, d);
#pragma unroll
            for (int j = 0; j < 3; ++j) t[j] += d[j];
        }
        double Vi[3][3];
        sym3(w.Vi + 6 * (int64_t)p, Vi);
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
__global__ __launch_bounds__(kThreads) void pcg_cg_camera_kernel(PnPCamera cam, const double* __restrict__ poses,
                                                                 const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave][6];
    __shared__ double total[6];
    if (w.st->stop || w.st->cg_done) return;
    const Chunk ch = camera_chunk(w);
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * (int64_t)ch.c + k];
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = ch.i0; i < ch.i1; ++i) {
        const int64_t p = w.pt_c[i];
        double Jc[2][6], Jp[2][3], e[6];
        if (!jacobians(m, cam, points[3 * p], points[3 * p + 1], points[3 * p + 2], Jc, Jp)) continue;
        w_times(Jc, Jp, w.y + 3 * p, e);
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] += e[k];
    }
    block_sum<6, kThreads>(a, part, total);
    if (threadIdx.x != 0) return;
    const int s = blockIdx.x;
    double A[6][6];
    damped_u(w.U + 21 * (int64_t)ch.c, w.st->lambda, A);
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
    __shared__ double part[kOneGroup / kWave][2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->stop || st->cg_done) return;
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
// (by camera, 0 for a fixed one) and the trial poses.  The free cameras' share of |delta|^2 and |x|^2.
__global__ __launch_bounds__(kOneGroup) void pcg_apply_kernel(int C, const double* __restrict__ poses, Ws w) {
    __shared__ double part[kOneGroup / kWave][2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->stop) return;
    const int k = st->cg_k;
    bool finite = true;
    for (int c = threadIdx.x; c < C; c += kOneGroup) {
        const int s = w.slot[c];
        if (s < 0) continue;
        for (int i = 0; i < 6; ++i) finite = finite && isfinite(w.x[6 * (int64_t)s + i]);
    }
    const bool ok = __syncthreads_and(finite) && !st->cg_fail;
    double v[2] = {0.0, 0.0};   // |dc|^2 | |t|^2
    for (int c = threadIdx.x; c < C; c += kOneGroup) {
        const int s = w.slot[c];
        const double* pose = poses + 12 * (int64_t)c;
        double* out = w.tpose + 12 * (int64_t)c;
        double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (s < 0 || !ok) {
            for (int i = 0; i < 12; ++i) out[i] = pose[i];
        } else {
            for (int i = 0; i < 6; ++i) d[i] = w.x[6 * (int64_t)s + i];
            apply_step(pose, d, out);
            for (int i = 0; i < 6; ++i) v[0] += d[i] * d[i];
            for (int i = 9; i < 12; ++i) v[1] += pose[i] * pose[i];
        }
        for (int i = 0; i < 6; ++i) w.dc[6 * (int64_t)c + i] = d[i];
    }
    block_sum<2, kOneGroup>(v, part, total);
    if (threadIdx.x != 0) return;
    st->step_ok = ok;
    st->dn_c = total[0];
    st->xn_c = total[1];
    st->cg_total += k;
    st->cg_max = max(st->cg_max, k);
}

// Thread per point: dX_p = V_p*^-1 (-g_p - sum over its free-camera observations of W^T dc), the trial point, the trial
// cost of its observations and its share of |delta|^2 and |x|^2; partials per block.
__global__ __launch_bounds__(kThreads) void pcg_trial_kernel(Obs obs, int P, PnPCamera cam, const double* __restrict__ poses,
                                                             const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave][3];
    __shared__ double total[3];
    if (w.st->stop || !w.st->step_ok) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};   // cost | |dX|^2 | |X|^2
    if (p < P) {
        double X[3] = {points[3 * (int64_t)p], points[3 * (int64_t)p + 1], points[3 * (int64_t)p + 2]};
        const int q0 = w.off_p[p], q1 = w.off_p[p + 1];
        if (q1 - q0 >= 2) {
            double t[3] = {-w.gp[3 * (int64_t)p], -w.gp[3 * (int64_t)p + 1], -w.gp[3 * (int64_t)p + 2]};
            for (int q = q0; q < q1; ++q) {
                const int c = w.camp[q];
                if (w.slot[c] < 0) continue;
                double Jc[2][6], Jp[2][3], d[3];
                if (!jacobians(poses + 12 * (int64_t)c, cam, X[0], X[1], X[2], Jc, Jp)) continue;
                wt_times(Jc, Jp, w.dc + 6 * (int64_t)c, d);
#pragma unroll
                for (int j = 0; j < 3; ++j) t[j] -= d[j];
            }
            double Vi[3][3];
            sym3(w.Vi + 6 * (int64_t)p, Vi);
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
        for (int i = 0; i < 3; ++i) w.tpts[3 * (int64_t)p + i] = X[i];
        for (int q = q0; q < q1; ++q) {
            const int64_t m = w.ord_p[q];
            a[0] += pnp_score(w.tpose + 12 * (int64_t)w.camp[q], cam, X[0], X[1], X[2], obs.uv[2 * m], obs.uv[2 * m + 1]);
        }
    }
    block_sum<3, kThreads>(a, part, total);
    if (threadIdx.x < 3) w.ppart[3 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

// Sums of the per-block partials in a fixed order (strided per thread, then block_sum).
template <int K>
SFM_DEVICE void sum_partials(const double* part, int blocks, double (*scratch)[3], double* total) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kOneGroup)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += part[3 * (int64_t)i + k];
    block_sum<K, kOneGroup>(v, reinterpret_cast<double(*)[K]>(scratch), total);
}

// After the first linearisation: the starting cost, the bad-start status, the gauge anchor (found on the host: the
// fixed camera f and the lowest free camera a when exactly one camera is fixed, else a = -1).
__global__ __launch_bounds__(kOneGroup) void pcg_start_kernel(int blocks, int f, int a, int max_steps,
                                                              const double* __restrict__ poses, Ws w) {
    __shared__ double scratch[kOneGroup / kWave][3];
    __shared__ double total[3];
    State* st = w.st;
    if (st->status != 0) return;
    sum_partials<1>(w.ppart, blocks, scratch, total);
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
        centre(poses + 12 * (int64_t)f, c0);
        centre(poses + 12 * (int64_t)a, ca);
        const double d0 = ca[0] - c0[0], d1 = ca[1] - c0[1], d2 = ca[2] - c0[2];
        st->dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        for (int k = 0; k < 3; ++k) st->c0[k] = c0[k];
    }
}

__global__ __launch_bounds__(kOneGroup) void pcg_decide_kernel(int blocks, int a, int max_steps, Ws w) {
    __shared__ double scratch[kOneGroup / kWave][3];
    __shared__ double total[3];
    State* st = w.st;
    const bool stop = st->stop, step_ok = st->step_ok;
    __syncthreads();   // every thread has read the state before thread 0 writes it
    if (threadIdx.x == 0) st->commit = 0;
    if (stop) return;
    if (step_ok) sum_partials<3>(w.ppart, blocks, scratch, total);   // block-uniform
    if (threadIdx.x != 0) return;
    st->steps += 1;
    st->fail = 0;
    st->cg_fail = 0;
    st->cg_done = 0;
    double lambda = st->lambda;
    bool done = false;
    if (!step_ok) {
        lambda *= 10.0;
    } else {
        const double dn = total[1] + st->dn_c, xn = total[2] + st->xn_c;
        const double c_new = total[0], c_old = st->cost;
        if (sqrt(dn) <= kMinStep * (1.0 + sqrt(xn))) {
            done = true;
        } else if (isfinite(c_new) && c_new < c_old) {
            done = c_old - c_new < kMinDecrease * c_old;
            st->cost = c_new;
            st->accepted += 1;
            st->commit = 1;
            st->need_lin = 1;
            lambda /= 10.0;
            if (a >= 0) {
                double ca[3];
                centre(w.tpose + 12 * (int64_t)a, ca);
                const double d0 = ca[0] - st->c0[0], d1 = ca[1] - st->c0[1], d2 = ca[2] - st->c0[2];
                st->scale = st->dist / sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            }
        } else {
            lambda *= 10.0;
        }
    }
    st->lambda = lambda;
    st->stop = done || st->steps >= max_steps || lambda > kLambdaMax;
}

// An accepted trial becomes the current estimate; with one fixed camera (a >= 0), scaled about its centre by st->scale.
// Thread i takes point i and camera i.
__global__ __launch_bounds__(kThreads) void pcg_commit_kernel(int P, int C, int a, double* __restrict__ poses,
                                                              double* __restrict__ points, Ws w) {
    const State* st = w.st;
    if (!st->commit) return;
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
            centre(tp, cc);
            for (int k = 0; k < 3; ++k) cc[k] = c0[k] + s * (cc[k] - c0[k]);
            for (int r = 0; r < 3; ++r) out[9 + r] = -((tp[3 * r] * cc[0] + tp[3 * r + 1] * cc[1]) + tp[3 * r + 2] * cc[2]);
        } else {
            for (int r = 0; r < 3; ++r) out[9 + r] = tp[9 + r];
        }
    }
}

__global__ void pcg_finish_kernel(Ws w, sfm_bundle_pcg_info* __restrict__ info) {
    const State* st = w.st;
    const bool bad_index = st->status == SFM_BUNDLE_BAD_INDEX;
    info->initial_cost = bad_index ? NAN : st->initial_cost;
    info->final_cost = bad_index ? NAN : st->cost;
    info->steps = st->steps;
    info->accepted = st->accepted;
    info->status = st->status;
    info->cg_iterations = st->cg_total;
    info->cg_max = st->cg_max;
    info->reserved = 0;
}

// Exclusive scan of n counts in place (off[0 .. n), off[n] = their total) by the point order's three scan levels.  Its
// level 3 also writes `fill`, here the same array: both stores of a thread carry the same value.
void launch_scan(int32_t* counts, int64_t n, int32_t* tile_sum, int32_t* flag, hipStream_t st) {
    const sfmorder::PointOrder o{counts, counts, nullptr, tile_sum, flag};
    const int T = (int)sfmorder::tiles(n);
    hipLaunchKernelGGL(sfmorder::order_scan_tiles_kernel, dim3((unsigned)T), dim3(sfmorder::kThreads), 0, st, (int)n, o);
    hipLaunchKernelGGL(sfmorder::order_scan_totals_kernel, dim3(1), dim3(sfmorder::kTotalsThreads), 0, st, (int)n, T, o);
    hipLaunchKernelGGL(sfmorder::order_scan_add_kernel, dim3(sfmhost::grid_for(n, sfmorder::kThreads)),
                       dim3(sfmorder::kThreads), 0, st, (int)n, o);
}

// The host's copy of the two flags {stop, cg_done}: pinned, one per host thread, allocated on its first call and kept.
int32_t* pinned_flags() {
    thread_local int32_t* flags = nullptr;
    if (!flags && hipHostMalloc(reinterpret_cast<void**>(&flags), 2 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
        flags = nullptr;
    return flags;
}

}  // namespace

extern "C" {

int64_t sfm_bundle_pcg_workspace_bytes(int64_t cameras, int64_t points, int64_t observations) {
    if (cameras < 1 || points < 0 || observations < 0 || cameras > 0x7FFFFFFF || points > 0x7FFFFFFF ||
        observations > 0x7FFFFFFF)
        return -1;
    return (int64_t)layout(cameras, points, observations, cameras - 1).total;
}

int sfm_bundle_adjust_pcg(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                          const double* poses_in, const double* points_in, const int32_t* camera_index,
                          const int32_t* point_index, const double* pixels, int max_steps, int max_cg_iterations,
                          double cg_tolerance, double* poses_out, double* points_out, sfm_bundle_pcg_info* info,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (cameras < 1 || points < 0 || observations < 0 || max_steps < 0)
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: bad size");
    if (cameras > 0x7FFFFFFF || points > 0x7FFFFFFF || observations > 0x7FFFFFFF)
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: cameras, points and observations must be below 2^31");
    if (max_cg_iterations < 1) return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: max_cg_iterations must be at least 1");
    if (!(cg_tolerance > 0.0 && cg_tolerance < 1.0))
        return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: cg_tolerance must be finite and in (0, 1)");
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
    const Layout L = layout(C, P, M, F);
    if (workspace_bytes < (int64_t)L.total) return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_bundle_adjust_pcg: workspace must be 16-byte aligned");
    int32_t* flags = pinned_flags();
    if (!flags) return fail(SFM_EHIP, "sfm_bundle_adjust_pcg: no pinned host memory for the flags");

    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(workspace, L);
    const Obs obs{camera_index, point_index, pixels};
    const int anchor = C - F == 1 && F > 0 ? (int)first_free : -1;   // one fixed camera: the gauge anchor
    const unsigned pgrid = sfmhost::grid_for(P, kThreads), cgrid = sfmhost::grid_for(C, kThreads);
    const unsigned mgrid = sfmhost::grid_for(M, kThreads), m1grid = sfmhost::grid_for(M + 1, kThreads);
    const unsigned icgrid = sfmhost::grid_for(P > C ? P : C, kThreads);
    const int pblocks = (int)((P + kThreads - 1) / kThreads);
    const int rtiles = (int)radix_tiles(M);
    // reads {stop, cg_done} into the pinned flags (synchronises the stream)
    auto read_flags = [&]() -> int {
        if (hipMemcpyAsync(flags, &w.st->stop, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
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
    if (hipMemcpyAsync(w.slot, slot.data(), 4 * C, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(w.off_p, 0, 4 * (P + 1), st) != hipSuccess)
        return check_launch("sfm_bundle_adjust_pcg: set up the workspace");
    hipLaunchKernelGGL(pcg_init_kernel, dim3(cgrid), dim3(kThreads), 0, st, (int)C, w);
    sfmorder::launch_point_order(camera_index, point_index, M, C, P,
                                 sfmorder::PointOrder{w.off_p, w.fill_p, w.ord_p, w.tsum_p, &w.st->bad}, st);
    hipLaunchKernelGGL(pcg_positions_kernel, dim3(mgrid), dim3(kThreads), 0, st, obs, (int)M, w);
    int32_t *src = w.seq0, *dst = w.seq1;
    for (int shift = 0; M > 0 && ((C - 1) >> shift) > 0; shift += kRadixBits) {
        hipLaunchKernelGGL(pcg_radix_kernel<false>, dim3(rtiles), dim3(kRadixTile), 0, st, (int)M, shift, rtiles, src, dst, w);
        launch_scan(w.table, (int64_t)kDigits * rtiles, w.tsum_r, &w.st->bad, st);
        hipLaunchKernelGGL(pcg_radix_kernel<true>, dim3(rtiles), dim3(kRadixTile), 0, st, (int)M, shift, rtiles, src, dst, w);
        int32_t* t = src;
        src = dst;
        dst = t;
    }
    hipLaunchKernelGGL(pcg_camera_order_kernel, dim3(m1grid), dim3(kThreads), 0, st, obs, (int)M, (int)C, src, w);
    hipLaunchKernelGGL(pcg_linearize_kernel, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, poses_out, points_out, w);
    if (F > 0)
        hipLaunchKernelGGL(pcg_camera_kernel, dim3((unsigned)F), dim3(kThreads), 0, st, obs, cam, poses_out, points_out, w);
    hipLaunchKernelGGL(pcg_start_kernel, dim3(1), dim3(kOneGroup), 0, st, pblocks, (int)first_fixed, anchor, max_steps,
                       poses_out, w);
    for (int step = 0; step < max_steps; ++step) {
        int rc2 = read_flags();   // also the point after which the host slots may go
        if (rc2 != SFM_OK) return rc2;
        if (flags[0]) break;
        hipLaunchKernelGGL(pcg_linearize_kernel, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, poses_out,
                           points_out, w);
        if (F > 0)
            hipLaunchKernelGGL(pcg_camera_kernel, dim3((unsigned)F), dim3(kThreads), 0, st, obs, cam, poses_out, points_out, w);
        hipLaunchKernelGGL(pcg_point_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, w);
        if (F > 0)
            hipLaunchKernelGGL(pcg_precond_kernel, dim3((unsigned)F), dim3(kThreads), 0, st, cam, poses_out, points_out, w);
        hipLaunchKernelGGL(pcg_cg_init_kernel, dim3(1), dim3(kOneGroup), 0, st, (int)F, cg_tolerance, w);
        for (int k0 = 0; F > 0 && k0 < max_cg_iterations; k0 += kCgChunk) {
            if (k0 > 0) {
                rc2 = read_flags();
                if (rc2 != SFM_OK) return rc2;
                if (flags[0] || flags[1]) break;
            }
            for (int k = k0; k < max_cg_iterations && k < k0 + kCgChunk; ++k) {
                hipLaunchKernelGGL(pcg_cg_point_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, cam, poses_out,
                                   points_out, w);
                hipLaunchKernelGGL(pcg_cg_camera_kernel, dim3((unsigned)F), dim3(kThreads), 0, st, cam, poses_out,
                                   points_out, w);
                hipLaunchKernelGGL(pcg_cg_update_kernel, dim3(1), dim3(kOneGroup), 0, st, (int)F, max_cg_iterations, w);
            }
        }
        hipLaunchKernelGGL(pcg_apply_kernel, dim3(1), dim3(kOneGroup), 0, st, (int)C, poses_out, w);
        hipLaunchKernelGGL(pcg_trial_kernel, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, poses_out, points_out, w);
        hipLaunchKernelGGL(pcg_decide_kernel, dim3(1), dim3(kOneGroup), 0, st, pblocks, anchor, max_steps, w);
        hipLaunchKernelGGL(pcg_commit_kernel, dim3(icgrid), dim3(kThreads), 0, st, (int)P, (int)C, anchor, poses_out,
                           points_out, w);
    }
    hipLaunchKernelGGL(pcg_finish_kernel, dim3(1), dim3(1), 0, st, w, info);
    if (max_steps == 0) {   // no read above: the host slots must reach the device before they go
        const int rc2 = read_flags();
        if (rc2 != SFM_OK) return rc2;
    }
    return check_launch("sfm_bundle_adjust_pcg");
}

}  // extern "C"
