// Bundle adjustment: Levenberg-Marquardt over C <= 64 camera poses and P points on the sum of the PnP scorer's squared
// reprojection errors, with the Schur complement on the points (the NumPy oracle is tests/bundle_oracle.py).
// fp64 throughout; off unless asked for.
//
// Set-up, once per call: the observations in point-major order (a counting sort by point; each point's run then sorted by
// observation index, so the order does not depend on atomics) and in camera-major order (a stable counting sort of the
// point-major order by camera: inside a camera the observations are sorted by point, which the merge-joins of the
// reduced camera system walk).  Then per LM trial step, every launch reading the LM state in the workspace first and
// returning at once after a stop:
//   bundle_linearize_kernel   (only after an accepted step)  thread per point: V_p, g_p, and W = Jc^T Jp per observation
//   bundle_camera_kernel      (only after an accepted step)  block per free camera: U_c and g_c over its observations
//   bundle_point_kernel       thread per point: V_p* = V_p + lambda diag V_p and its inverse
//   bundle_schur_kernel       block per upper block (a, b) of free cameras: sum_p W_ap V_p*^-1 W_bp^T by a merge-join of
//                             the two cameras' point-sorted lists (and the right-hand side term on the diagonal blocks)
//   bundle_solve_kernel       one workgroup: dense Cholesky of S (6F x 6F, in LDS up to kLdsFree free cameras), both
//                             triangular solves, the camera steps and the trial poses
//   bundle_trial_kernel       thread per point: back-substitution dX_p, the trial point, its observations' trial cost
//   bundle_decide_kernel      one workgroup: the cost in a fixed order, accept / reject, lambda, the gauge scale, stops
//   bundle_commit_kernel      an accepted trial becomes the current estimate (rescaled when one camera is fixed)
// No floating-point atomics anywhere: every sum runs in an order fixed by the sizes alone, so a call is bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_pnp.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmpnp::camera_from;
using sfmpnp::pnp_score;
using sfmpnp::PnPCamera;

constexpr int kMaxCameras = 64;
constexpr int kLdsFree = 30;                 // S (packed lower triangle) in LDS up to this many free cameras: 127 KiB
constexpr int kThreads = 256;                // point-parallel and per-block kernels
constexpr int kSolveThreads = 1024;          // the one-workgroup solve
constexpr int kTile = 1024;                  // observations per block of the camera-major counting sort
constexpr int kMaxSolve = 6 * (kMaxCameras - 1);
constexpr double kLambda0 = 1e-3;
constexpr double kLambdaMax = 1e16;
constexpr double kMinDecrease = 1e-12;
constexpr double kMinStep = 1e-12;

static_assert(sizeof(sfm_bundle_info) == 32, "sfm_bundle_info layout is part of the ABI");

// The LM state: written by one thread of the start / solve / decide kernels, read by every launch after it.
struct State {
    double lambda, cost, initial_cost, scale;
    double c0[3], dist;     // gauge: the fixed camera's centre and the anchor camera's distance from it
    int32_t steps, accepted, status, stop;
    int32_t need_lin;       // the current estimate has no linearisation yet (start, or an accepted step)
    int32_t step_ok;        // the damped system factored and the step is finite
    int32_t commit;         // this step's trial was accepted
    int32_t fail;           // a V_p* did not factor (set by any thread of bundle_point_kernel)
    int32_t anchor;         // lowest free camera when exactly one camera is fixed, else -1
    int32_t pad[3];
};

struct Layout {
    size_t state, off_p, fill_p, off_c, ord_p, ord_c, pt_c, tiles, W, V, gp, Vi, U, gc, blk, rhs, S, dc, tpose, tpts, part,
        total;
};

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

Layout layout(int64_t C, int64_t P, int64_t M) {
    Layout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o = align256(o + bytes);
        return (size_t)at;
    };
    const int64_t F = C > 0 ? C - 1 : 0;   // at least one camera is fixed
    const int64_t tiles = (M + kTile - 1) / kTile;
    const int64_t pblocks = (P + kThreads - 1) / kThreads;
    L.state = take(sizeof(State));
    L.off_p = take(4 * (P + 1));
    L.fill_p = take(4 * P);
    L.off_c = take(4 * (C + 1) * 2);   // offsets | counts
    L.ord_p = take(4 * M);
    L.ord_c = take(4 * M);
    L.pt_c = take(4 * M);
    L.tiles = take(4 * C * tiles);
    L.W = take(8 * 18 * M);
    L.V = take(8 * 6 * P);
    L.gp = take(8 * 3 * P);
    L.Vi = take(8 * 6 * P);
    L.U = take(8 * 21 * C);
    L.gc = take(8 * 6 * C);
    L.blk = take(8 * 36 * (F * (F + 1) / 2));
    L.rhs = take(8 * 6 * C);
    L.S = take(F > kLdsFree ? 8 * (6 * F) * (6 * F + 1) / 2 : 0);
    L.dc = take(8 * 6 * C);
    L.tpose = take(8 * 12 * C);
    L.tpts = take(8 * 3 * P);
    L.part = take(8 * 3 * (pblocks > 0 ? pblocks : 1));
    L.total = (size_t)o;
    return L;
}

struct Ws {
    State* st;
    int32_t *off_p, *fill_p, *off_c, *ord_p, *ord_c, *pt_c, *tiles;
    double *W, *V, *gp, *Vi, *U, *gc, *blk, *rhs, *S, *dc, *tpose, *tpts, *part;
};

Ws carve(void* base, const Layout& L) {
    char* b = static_cast<char*>(base);
    Ws w;
    w.st = reinterpret_cast<State*>(b + L.state);
    w.off_p = reinterpret_cast<int32_t*>(b + L.off_p);
    w.fill_p = reinterpret_cast<int32_t*>(b + L.fill_p);
    w.off_c = reinterpret_cast<int32_t*>(b + L.off_c);
    w.ord_p = reinterpret_cast<int32_t*>(b + L.ord_p);
    w.ord_c = reinterpret_cast<int32_t*>(b + L.ord_c);
    w.pt_c = reinterpret_cast<int32_t*>(b + L.pt_c);
    w.tiles = reinterpret_cast<int32_t*>(b + L.tiles);
    w.W = reinterpret_cast<double*>(b + L.W);
    w.V = reinterpret_cast<double*>(b + L.V);
    w.gp = reinterpret_cast<double*>(b + L.gp);
    w.Vi = reinterpret_cast<double*>(b + L.Vi);
    w.U = reinterpret_cast<double*>(b + L.U);
    w.gc = reinterpret_cast<double*>(b + L.gc);
    w.blk = reinterpret_cast<double*>(b + L.blk);
    w.rhs = reinterpret_cast<double*>(b + L.rhs);
    w.S = reinterpret_cast<double*>(b + L.S);
    w.dc = reinterpret_cast<double*>(b + L.dc);
    w.tpose = reinterpret_cast<double*>(b + L.tpose);
    w.tpts = reinterpret_cast<double*>(b + L.tpts);
    w.part = reinterpret_cast<double*>(b + L.part);
    return w;
}

// The observations: camera and point index, pixel.
struct Obs {
    const int32_t* cam;
    const int32_t* pt;
    const double* uv;
};

SFM_DEVICE bool is_fixed(uint64_t fixed, int c) { return (fixed >> c) & 1ull; }

// Slot s of the free cameras -> camera index (the s-th zero bit of `fixed`).
SFM_DEVICE int free_camera(uint64_t fixed, int C, int s) {
    for (int c = 0; c < C; ++c)
        if (!is_fixed(fixed, c) && s-- == 0) return c;
    return -1;
}

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

// Residual r, c = R X + t and the Jacobian rows of one observation in front of the camera (the rows of
// sfm_pnp_refine.hip's accumulate: row k of Jc = (R X x A_k, A_k), and of Jp = A_k R).  False behind the camera.
SFM_DEVICE bool linearize(const double* m, const PnPCamera& k, double X, double Y, double Z, double u, double v,
                          double (&r)[2], double (&Jc)[2][6], double (&Jp)[2][3]) {
    const double r0 = (m[0] * X + m[1] * Y) + m[2] * Z;
    const double r1 = (m[3] * X + m[4] * Y) + m[5] * Z;
    const double r2 = (m[6] * X + m[7] * Y) + m[8] * Z;
    const double c0 = r0 + m[9], c1 = r1 + m[10], c2 = r2 + m[11];
    if (!(c2 > 0.0)) return false;
    const double w0 = ((k.k00 * c0 + k.k01 * c1) + k.k02 * c2) / c2;
    const double w1 = ((k.k10 * c0 + k.k11 * c1) + k.k12 * c2) / c2;
    r[0] = w0 - u;
    r[1] = w1 - v;
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

SFM_DEVICE int upper6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }   // r <= c, 21 entries
SFM_DEVICE int upper3(int r, int c) { return r * 3 - r * (r - 1) / 2 + (c - r); }   // r <= c, 6 entries
SFM_DEVICE int64_t lower(int i, int j) { return (int64_t)i * (i + 1) / 2 + j; }      // i >= j, packed lower triangle

// out = {exp([w]x) R | t + dt}: Rodrigues with the Taylor forms of sfm_pnp_refine.hip below th = 1e-6.
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

__global__ void bundle_init_kernel(Ws w) {
    State s{};
    s.lambda = kLambda0;
    s.need_lin = 1;
    s.anchor = -1;
    *w.st = s;
}

// ------------------------------------------------------------------------------------------------------------------------
// Set-up: index check and counts, offsets, the point-major and the camera-major orders.
// ------------------------------------------------------------------------------------------------------------------------
// Cameras are counted in LDS first (one global atomic per block and camera): 64 global counters shared by millions of
// observations would serialise.
__global__ __launch_bounds__(kThreads) void bundle_count_kernel(Obs obs, int M, int C, int P, Ws w) {
    __shared__ int32_t per_camera[kMaxCameras];
    if (threadIdx.x < kMaxCameras) per_camera[threadIdx.x] = 0;
    __syncthreads();
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m < M) {
        const int c = obs.cam[m], p = obs.pt[m];
        if (c < 0 || c >= C || p < 0 || p >= P) {   // every offender stores the same values
            w.st->status = SFM_BUNDLE_BAD_INDEX;
            w.st->stop = 1;
        } else {
            atomicAdd(w.off_p + p, 1);
            atomicAdd(per_camera + c, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < C && per_camera[threadIdx.x] != 0) atomicAdd(w.off_c + (C + 1) + threadIdx.x, per_camera[threadIdx.x]);
}

// counts -> exclusive offsets for the points (in place, chunked over one workgroup) and the cameras; fill_p = off_p
__global__ __launch_bounds__(kSolveThreads) void bundle_scan_kernel(int C, int P, int M, Ws w) {
    __shared__ int32_t sums[kSolveThreads];
    if (w.st->status != 0) return;
    const int tid = threadIdx.x;
    const int64_t chunk = ((int64_t)P + kSolveThreads - 1) / kSolveThreads;
    const int64_t lo = min((int64_t)P, tid * chunk), hi = min((int64_t)P, lo + chunk);
    int32_t s = 0;
    for (int64_t p = lo; p < hi; ++p) s += w.off_p[p];
    sums[tid] = s;
    __syncthreads();
    for (int off = 1; off < kSolveThreads; off <<= 1) {
        const int32_t below = tid >= off ? sums[tid - off] : 0;
        __syncthreads();
        sums[tid] += below;
        __syncthreads();
    }
    int32_t run = sums[tid] - s;
    for (int64_t p = lo; p < hi; ++p) {
        const int32_t n = w.off_p[p];
        w.off_p[p] = run;
        w.fill_p[p] = run;
        run += n;
    }
    if (tid == 0) {
        w.off_p[P] = M;
        int32_t acc = 0;
        for (int c = 0; c < C; ++c) {
            w.off_c[c] = acc;
            acc += w.off_c[C + 1 + c];
        }
        w.off_c[C] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void bundle_scatter_points_kernel(Obs obs, int M, Ws w) {
    if (w.st->status != 0) return;
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    w.ord_p[atomicAdd(w.fill_p + obs.pt[m], 1)] = m;
}

// each point's run sorted by observation index (insertion sort: runs hold a few observations)
__global__ __launch_bounds__(kThreads) void bundle_sort_runs_kernel(int P, Ws w) {
    if (w.st->status != 0) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    int32_t* run = w.ord_p + w.off_p[p];
    const int n = w.off_p[p + 1] - w.off_p[p];
    for (int i = 1; i < n; ++i) {
        const int32_t v = run[i];
        int j = i - 1;
        while (j >= 0 && run[j] > v) {
            run[j + 1] = run[j];
            --j;
        }
        run[j + 1] = v;
    }
}

// Stable counting sort of the point-major order by camera, tile by tile.  Rank of a position among the tile's positions of
// the same camera: a ballot per camera inside each wave, then the waves in order.
struct TileRanks {
    int key, rank;
};

SFM_DEVICE TileRanks tile_ranks(const Obs& obs, const Ws& w, int M, int C, int32_t (*wcount)[kMaxCameras]) {
    const int q = blockIdx.x * kTile + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int key = q < M ? obs.cam[w.ord_p[q]] : -1;
    int rank = 0;
    for (int c = 0; c < C; ++c) {
        const uint64_t b = __ballot(key == c);
        if (key == c) rank = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[wave][c] = __popcll(b);
    }
    __syncthreads();
    return TileRanks{key, rank};
}

__global__ __launch_bounds__(kTile) void bundle_tile_count_kernel(Obs obs, int M, int C, int tiles, Ws w) {
    __shared__ int32_t wcount[kTile / kWave][kMaxCameras];
    if (w.st->status != 0) return;
    tile_ranks(obs, w, M, C, wcount);
    if (threadIdx.x < C) {
        int32_t n = 0;
        for (int v = 0; v < kTile / kWave; ++v) n += wcount[v][threadIdx.x];
        w.tiles[(int64_t)threadIdx.x * tiles + blockIdx.x] = n;
    }
}

// tile counts -> the first output position of every (camera, tile); one wave per camera, 64 tiles per wave step
__global__ __launch_bounds__(kSolveThreads) void bundle_tile_scan_kernel(int C, int tiles, Ws w) {
    if (w.st->status != 0) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int c = wave; c < C; c += kSolveThreads / kWave) {
        int32_t* row = w.tiles + (int64_t)c * tiles;
        int32_t run = w.off_c[c];
        for (int t0 = 0; t0 < tiles; t0 += kWave) {
            const int t = t0 + lane;
            const int32_t own = t < tiles ? row[t] : 0;
            int32_t inc = own;
            for (int off = 1; off < kWave; off <<= 1) {
                const int32_t below = __shfl_up(inc, off, kWave);
                if (lane >= off) inc += below;
            }
            if (t < tiles) row[t] = run + inc - own;
            run += __shfl(inc, kWave - 1, kWave);
        }
    }
}

__global__ __launch_bounds__(kTile) void bundle_tile_scatter_kernel(Obs obs, int M, int C, int tiles, Ws w) {
    __shared__ int32_t wcount[kTile / kWave][kMaxCameras];
    if (w.st->status != 0) return;
    const TileRanks r = tile_ranks(obs, w, M, C, wcount);
    if (r.key < 0) return;
    const int wave = threadIdx.x / kWave;
    int32_t before = 0;
    for (int v = 0; v < wave; ++v) before += wcount[v][r.key];
    const int q = blockIdx.x * kTile + threadIdx.x;
    const int32_t pos = w.tiles[(int64_t)r.key * tiles + blockIdx.x] + before + r.rank;
    w.ord_c[pos] = q;
    w.pt_c[pos] = obs.pt[w.ord_p[q]];
}

// ------------------------------------------------------------------------------------------------------------------------
// Linearisation.
// ------------------------------------------------------------------------------------------------------------------------
SFM_DEVICE void load_poses(const double* src, int C, double* dst) {
    for (int k = threadIdx.x; k < 12 * C; k += kThreads) dst[k] = src[k];
    __syncthreads();
}

// Thread per point: the cost of its observations (partial per block; the start needs it), V_p, g_p, and W for each of its
// observations by a free camera when the point moves.
__global__ __launch_bounds__(kThreads) void bundle_linearize_kernel(Obs obs, int P, PnPCamera cam, uint64_t fixed,
                                                                   const double* __restrict__ poses,
                                                                   const double* __restrict__ points, int C, Ws w) {
    __shared__ double pose[kMaxCameras * 12];
    __shared__ double part[kThreads / kWave][1];
    __shared__ double total[1];
    if (w.st->stop || !w.st->need_lin) return;
    load_poses(poses, C, pose);
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double e[1] = {0.0};
    if (p < P) {
        const double X = points[3 * (int64_t)p], Y = points[3 * (int64_t)p + 1], Z = points[3 * (int64_t)p + 2];
        const int q0 = w.off_p[p], q1 = w.off_p[p + 1];
        const bool moving = q1 - q0 >= 2;
        double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        for (int q = q0; q < q1; ++q) {
            const int m = w.ord_p[q];
            const int c = obs.cam[m];
            const double* mp = pose + 12 * c;
            const double u = obs.uv[2 * (int64_t)m], v = obs.uv[2 * (int64_t)m + 1];
            e[0] += pnp_score(mp, cam, X, Y, Z, u, v);
            double r[2], Jc[2][6], Jp[2][3];
            if (!linearize(mp, cam, X, Y, Z, u, v, r, Jc, Jp)) continue;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = i; j < 3; ++j) V[upper3(i, j)] += Jp[0][i] * Jp[0][j] + Jp[1][i] * Jp[1][j];
                g[i] += Jp[0][i] * r[0] + Jp[1][i] * r[1];
            }
            if (moving && !is_fixed(fixed, c)) {
                double* Wq = w.W + 18 * (int64_t)q;
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
    }
    block_sum<1, kThreads>(e, part, total);
    if (threadIdx.x == 0) w.part[3 * (int64_t)blockIdx.x] = total[0];
}

// Block per free camera: U_c (upper 21) and g_c over its observations in camera-major order.
__global__ __launch_bounds__(kThreads) void bundle_camera_kernel(Obs obs, PnPCamera cam, uint64_t fixed,
                                                                 const double* __restrict__ poses,
                                                                 const double* __restrict__ points, Ws w) {
    __shared__ double part[kThreads / kWave][27];
    __shared__ double total[27];
    const int c = blockIdx.x;
    if (w.st->stop || !w.st->need_lin || is_fixed(fixed, c)) return;
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = poses[12 * c + k];
    double a[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) a[k] = 0.0;
    const int lo = w.off_c[c], n = w.off_c[c + 1] - lo;
    const int chunk = (n + kThreads - 1) / kThreads;
    const int i0 = lo + min(n, (int)threadIdx.x * chunk), i1 = lo + min(n, ((int)threadIdx.x + 1) * chunk);
    for (int i = i0; i < i1; ++i) {
        const int mo = w.ord_p[w.ord_c[i]];
        const int64_t p = w.pt_c[i];
        double r[2], Jc[2][6], Jp[2][3];
        if (!linearize(m, cam, points[3 * p], points[3 * p + 1], points[3 * p + 2], obs.uv[2 * (int64_t)mo],
                       obs.uv[2 * (int64_t)mo + 1], r, Jc, Jp))
            continue;
#pragma unroll
        for (int x = 0; x < 6; ++x) {
#pragma unroll
            for (int y = x; y < 6; ++y) a[upper6(x, y)] += Jc[0][x] * Jc[0][y] + Jc[1][x] * Jc[1][y];
            a[21 + x] += Jc[0][x] * r[0] + Jc[1][x] * r[1];
        }
    }
    block_sum<27, kThreads>(a, part, total);
    if (threadIdx.x < 21) w.U[21 * c + threadIdx.x] = total[threadIdx.x];
    else if (threadIdx.x < 27) w.gc[6 * c + threadIdx.x - 21] = total[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------------
// One LM trial step.
// ------------------------------------------------------------------------------------------------------------------------
// Thread per moving point: V_p* = V_p + lambda diag V_p, its 3 x 3 Cholesky, and V_p*^-1 (upper 6).  A pivot <= 0 or not
// finite marks the step as failed.
__global__ __launch_bounds__(kThreads) void bundle_point_kernel(int P, Ws w) {
    if (w.st->stop) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P || w.off_p[p + 1] - w.off_p[p] < 2) return;
    const double lambda = w.st->lambda;
    const double* v = w.V + 6 * (int64_t)p;
    double A[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) A[i][j] = A[j][i] = v[upper3(i, j)];
#pragma unroll
    for (int i = 0; i < 3; ++i) A[i][i] = A[i][i] + lambda * A[i][i];
    // L L^T = A
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
    // A^-1 = L^-T L^-1: columns of L^-1 by forward substitution, then the products
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

SFM_DEVICE void sym3(const double* u, double (&A)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) A[i][j] = A[j][i] = u[upper3(i, j)];
}

// Block per upper block (a, b), a <= b, of the free cameras' slots: blk = sum over pairs (i in a, j in b) of observations
// of the same moving point p of W_i V_p*^-1 W_j^T.  Thread t takes a contiguous chunk of a's list and walks b's list
// beside it from a binary search.  On the diagonal blocks also rhs_a = sum_i W_i V_p*^-1 g_p.
__global__ __launch_bounds__(kThreads) void bundle_schur_kernel(uint64_t fixed, int C, Ws w) {
    __shared__ double part[kThreads / kWave][42];
    __shared__ double total[42];
    if (w.st->stop || w.st->fail) return;
    // block -> (a, b) in row-major order of the upper triangle
    const int F = C - __popcll(fixed);
    int a = 0, idx = blockIdx.x;
    while (idx >= F - a) {
        idx -= F - a;
        ++a;
    }
    const int b = a + idx;
    const int ca = free_camera(fixed, C, a), cb = free_camera(fixed, C, b);
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; ++k) acc[k] = 0.0;
    const int alo = w.off_c[ca], na = w.off_c[ca + 1] - alo;
    const int blo = w.off_c[cb], bhi = w.off_c[cb + 1];
    const int chunk = (na + kThreads - 1) / kThreads;
    const int i0 = alo + min(na, (int)threadIdx.x * chunk), i1 = alo + min(na, ((int)threadIdx.x + 1) * chunk);
    if (i0 < i1) {
        int j = blo, hi = bhi;   // first entry of b's list with point >= the chunk's first point
        const int32_t first = w.pt_c[i0];
        while (j < hi) {
            const int mid = (j + hi) >> 1;
            if (w.pt_c[mid] < first) j = mid + 1;
            else hi = mid;
        }
        for (int i = i0; i < i1; ++i) {
            const int32_t p = w.pt_c[i];
            if (w.off_p[p + 1] - w.off_p[p] < 2) continue;
            while (j < bhi && w.pt_c[j] < p) ++j;
            if (j >= bhi) break;
            if (w.pt_c[j] != p) continue;
            double Vi[3][3];
            sym3(w.Vi + 6 * (int64_t)p, Vi);
            const double* Wi = w.W + 18 * (int64_t)w.ord_c[i];
            double Y[6][3];
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y) Y[x][y] = (Wi[3 * x] * Vi[0][y] + Wi[3 * x + 1] * Vi[1][y]) + Wi[3 * x + 2] * Vi[2][y];
            for (int k = j; k < bhi && w.pt_c[k] == p; ++k) {
                const double* Wj = w.W + 18 * (int64_t)w.ord_c[k];
#pragma unroll
                for (int x = 0; x < 6; ++x)
#pragma unroll
                    for (int y = 0; y < 6; ++y) acc[6 * x + y] += (Y[x][0] * Wj[3 * y] + Y[x][1] * Wj[3 * y + 1]) + Y[x][2] * Wj[3 * y + 2];
            }
            if (a == b) {
                const double* g = w.gp + 3 * (int64_t)p;
#pragma unroll
                for (int x = 0; x < 6; ++x) acc[36 + x] += (Y[x][0] * g[0] + Y[x][1] * g[1]) + Y[x][2] * g[2];
            }
        }
    }
    block_sum<42, kThreads>(acc, part, total);
    if (threadIdx.x < 36) w.blk[36 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
    else if (a == b && threadIdx.x < 42) w.rhs[6 * a + threadIdx.x - 36] = total[threadIdx.x];
}

// One workgroup: S = U* - blk (lower triangle, packed), right-hand side -g_c + rhs, Cholesky, both triangular solves;
// then the camera steps and the trial poses.  S lives in LDS (kLds) or in the workspace.
template <bool kLds>
__global__ __launch_bounds__(kSolveThreads) void bundle_solve_kernel(uint64_t fixed, int C, const double* __restrict__ poses,
                                                                     Ws w) {
    constexpr int kLdsN = 6 * kLdsFree;
    __shared__ double lds[kLds ? kLdsN * (kLdsN + 1) / 2 : 1];
    __shared__ double y[kMaxSolve];
    __shared__ int ok;
    State* st = w.st;
    if (st->stop) return;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int kWaves = kSolveThreads / kWave;
    if (tid == 0) st->need_lin = 0;   // the linearisation kernels of this step have run
    const int F = C - __popcll(fixed), n = 6 * F;
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
                const int c = free_camera(fixed, C, a);
                const double u = w.U[21 * c + upper6(r, s)];
                v += r == s ? u + lambda * u : u;
            }
            A[e] = v;
        }
        for (int i = tid; i < n; i += kSolveThreads) {
            const int c = free_camera(fixed, C, i / 6);
            y[i] = -w.gc[6 * c + i % 6] + w.rhs[i];
        }
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
    if (tid < C) {
        const int c = tid;
        double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double* out = w.tpose + 12 * c;
        if (is_fixed(fixed, c) || !ok) {
#pragma unroll
            for (int k = 0; k < 12; ++k) out[k] = poses[12 * c + k];
        } else {
            const int s = c - __popcll(fixed & ((1ull << c) - 1ull));   // slot of a free camera
#pragma unroll
            for (int k = 0; k < 6; ++k) d[k] = y[6 * s + k];
            apply_step(poses + 12 * c, d, out);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) w.dc[6 * c + k] = d[k];
    }
    if (tid == 0) st->step_ok = ok;
}

// Thread per point: dX_p = V_p*^-1 (-g_p - sum over its free-camera observations of W^T dc), the trial point, the trial cost
// of its observations and its share of |delta|^2 and |x|^2; partials per block.
__global__ __launch_bounds__(kThreads) void bundle_trial_kernel(Obs obs, int P, PnPCamera cam, uint64_t fixed,
                                                                const double* __restrict__ points, int C, Ws w) {
    __shared__ double pose[kMaxCameras * 12];
    __shared__ double dc[kMaxCameras * 6];
    __shared__ double part[kThreads / kWave][3];
    __shared__ double total[3];
    if (w.st->stop || !w.st->step_ok) return;
    load_poses(w.tpose, C, pose);
    for (int k = threadIdx.x; k < 6 * C; k += kThreads) dc[k] = w.dc[k];
    __syncthreads();
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};   // cost | |dX|^2 | |X|^2
    if (p < P) {
        double X[3] = {points[3 * (int64_t)p], points[3 * (int64_t)p + 1], points[3 * (int64_t)p + 2]};
        const int q0 = w.off_p[p], q1 = w.off_p[p + 1];
        if (q1 - q0 >= 2) {
            double t[3] = {-w.gp[3 * (int64_t)p], -w.gp[3 * (int64_t)p + 1], -w.gp[3 * (int64_t)p + 2]};
            for (int q = q0; q < q1; ++q) {
                const int c = obs.cam[w.ord_p[q]];
                if (is_fixed(fixed, c)) continue;
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
            sym3(w.Vi + 6 * (int64_t)p, Vi);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double d = (Vi[i][0] * t[0] + Vi[i][1] * t[1]) + Vi[i][2] * t[2];
                a[1] += d * d;
                a[2] += X[i] * X[i];
                X[i] += d;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) w.tpts[3 * (int64_t)p + i] = X[i];
        for (int q = q0; q < q1; ++q) {
            const int m = w.ord_p[q];
            a[0] += pnp_score(pose + 12 * obs.cam[m], cam, X[0], X[1], X[2], obs.uv[2 * (int64_t)m], obs.uv[2 * (int64_t)m + 1]);
        }
    }
    block_sum<3, kThreads>(a, part, total);
    if (threadIdx.x < 3) w.part[3 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

// Sums of the per-block partials in a fixed order (strided per thread, then block_sum).
template <int K>
SFM_DEVICE void sum_partials(const double* part, int blocks, double (*scratch)[3], double* total) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kThreads)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += part[3 * (int64_t)i + k];
    block_sum<K, kThreads>(v, reinterpret_cast<double(*)[K]>(scratch), total);
}

// After the first linearisation: the starting cost, the bad-start status, the gauge anchor.
__global__ __launch_bounds__(kThreads) void bundle_start_kernel(int blocks, uint64_t fixed, int C, int max_steps,
                                                                const double* __restrict__ poses, Ws w) {
    __shared__ double scratch[kThreads / kWave][3];
    __shared__ double total[3];
    State* st = w.st;
    if (st->status != 0) return;
    sum_partials<1>(w.part, blocks, scratch, total);
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
    if (__popcll(fixed) == 1 && C > 1) {
        const int f = __builtin_ctzll(fixed);
        const int a = free_camera(fixed, C, 0);
        double c0[3], ca[3];
        centre(poses + 12 * f, c0);
        centre(poses + 12 * a, ca);
        const double d0 = ca[0] - c0[0], d1 = ca[1] - c0[1], d2 = ca[2] - c0[2];
        st->dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        for (int k = 0; k < 3; ++k) st->c0[k] = c0[k];
        st->anchor = a;
    }
}

__global__ __launch_bounds__(kThreads) void bundle_decide_kernel(int blocks, uint64_t fixed, int C, int max_steps,
                                                                 const double* __restrict__ poses, Ws w) {
    __shared__ double scratch[kThreads / kWave][3];
    __shared__ double total[3];
    State* st = w.st;
    if (threadIdx.x == 0) st->commit = 0;
    if (st->stop) return;
    const bool step_ok = st->step_ok;
    if (step_ok) sum_partials<3>(w.part, blocks, scratch, total);   // block-uniform
    if (threadIdx.x != 0) return;
    st->steps += 1;
    st->fail = 0;
    double lambda = st->lambda;
    bool stop = false;
    if (!step_ok) {
        lambda *= 10.0;
    } else {
        double dn = total[1], xn = total[2];
        for (int c = 0; c < C; ++c) {
            if (is_fixed(fixed, c)) continue;
            for (int k = 0; k < 6; ++k) dn += w.dc[6 * c + k] * w.dc[6 * c + k];
            for (int k = 9; k < 12; ++k) xn += poses[12 * c + k] * poses[12 * c + k];
        }
        const double c_new = total[0], c_old = st->cost;
        if (sqrt(dn) <= kMinStep * (1.0 + sqrt(xn))) {
            stop = true;
        } else if (isfinite(c_new) && c_new < c_old) {
            stop = c_old - c_new < kMinDecrease * c_old;
            st->cost = c_new;
            st->accepted += 1;
            st->commit = 1;
            st->need_lin = 1;
            lambda /= 10.0;
            if (st->anchor >= 0) {
                double ca[3];
                centre(w.tpose + 12 * st->anchor, ca);
                const double d0 = ca[0] - st->c0[0], d1 = ca[1] - st->c0[1], d2 = ca[2] - st->c0[2];
                st->scale = st->dist / sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            }
        } else {
            lambda *= 10.0;
        }
    }
    st->lambda = lambda;
    st->stop = stop || st->steps >= max_steps || lambda > kLambdaMax;
}

// An accepted trial becomes the current estimate; with one fixed camera, scaled about its centre by st->scale.
__global__ __launch_bounds__(kThreads) void bundle_commit_kernel(int P, uint64_t fixed, int C, double* __restrict__ poses,
                                                                 double* __restrict__ points, Ws w) {
    const State* st = w.st;
    if (!st->commit) return;
    const bool rescale = st->anchor >= 0;
    const double s = st->scale, c0[3] = {st->c0[0], st->c0[1], st->c0[2]};
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < P) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double x = w.tpts[3 * (int64_t)p + i];
            points[3 * (int64_t)p + i] = rescale ? c0[i] + s * (x - c0[i]) : x;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < C && !is_fixed(fixed, threadIdx.x)) {
        const double* tp = w.tpose + 12 * threadIdx.x;
        double* out = poses + 12 * threadIdx.x;
        for (int k = 0; k < 9; ++k) out[k] = tp[k];
        if (rescale) {
            double cc[3];
            centre(tp, cc);
            for (int i = 0; i < 3; ++i) cc[i] = c0[i] + s * (cc[i] - c0[i]);
            for (int r = 0; r < 3; ++r) out[9 + r] = -((tp[3 * r] * cc[0] + tp[3 * r + 1] * cc[1]) + tp[3 * r + 2] * cc[2]);
        } else {
            for (int r = 0; r < 3; ++r) out[9 + r] = tp[9 + r];
        }
    }
}

__global__ void bundle_finish_kernel(Ws w, sfm_bundle_info* __restrict__ info) {
    const State* st = w.st;
    const bool bad_index = st->status == SFM_BUNDLE_BAD_INDEX;
    info->initial_cost = bad_index ? NAN : st->initial_cost;
    info->final_cost = bad_index ? NAN : st->cost;
    info->steps = st->steps;
    info->accepted = st->accepted;
    info->status = st->status;
    info->reserved = 0;
}

}  // namespace

extern "C" {

int64_t sfm_bundle_workspace_bytes(int64_t cameras, int64_t points, int64_t observations) {
    if (cameras < 1 || cameras > kMaxCameras || points < 0 || observations < 0 || points > 0x7FFFFFFF ||
        observations > 0x7FFFFFFF)
        return -1;
    return (int64_t)layout(cameras, points, observations).total;
}

int sfm_bundle_adjust(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                      const double* poses_in, const double* points_in, const int32_t* camera_index,
                      const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                      double* points_out, sfm_bundle_info* info, void* workspace, int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (cameras < 1 || points < 0 || observations < 0 || max_steps < 0) return fail(SFM_EINVAL, "sfm_bundle_adjust: bad size");
    if (cameras > kMaxCameras) return fail(SFM_EINVAL, "sfm_bundle_adjust: more than 64 cameras");
    if (points > 0x7FFFFFFF || observations > 0x7FFFFFFF)
        return fail(SFM_EINVAL, "sfm_bundle_adjust: points and observations must be below 2^31");
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
    const Layout L = layout(C, P, M);
    if (workspace_bytes < (int64_t)L.total) return fail(SFM_EINVAL, "sfm_bundle_adjust: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_bundle_adjust: workspace must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(workspace, L);
    const Obs obs{camera_index, point_index, pixels};
    const int F = (int)C - __builtin_popcountll(mask);
    const int tiles = (int)((M + kTile - 1) / kTile);
    const unsigned pgrid = sfmhost::grid_for(P, kThreads), mgrid = sfmhost::grid_for(M, kThreads);
    const int pblocks = (int)((P + kThreads - 1) / kThreads);
    const unsigned pairs = (unsigned)(F * (F + 1) / 2);

    // the output starts as the input; the state, the point counters and the camera counters start at zero
    if (poses_out != poses_in && hipMemcpyAsync(poses_out, poses_in, 8 * 12 * C, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return check_launch("sfm_bundle_adjust: copy poses");
    if (P > 0 && points_out != points_in &&
        hipMemcpyAsync(points_out, points_in, 8 * 3 * P, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return check_launch("sfm_bundle_adjust: copy points");
    if (hipMemsetAsync(w.off_p, 0, 4 * (P + 1), st) != hipSuccess || hipMemsetAsync(w.off_c, 0, 8 * (C + 1), st) != hipSuccess)
        return check_launch("sfm_bundle_adjust: clear the counters");
    hipLaunchKernelGGL(bundle_init_kernel, dim3(1), dim3(1), 0, st, w);
    hipLaunchKernelGGL(bundle_count_kernel, dim3(mgrid), dim3(kThreads), 0, st, obs, (int)M, (int)C, (int)P, w);
    hipLaunchKernelGGL(bundle_scan_kernel, dim3(1), dim3(kSolveThreads), 0, st, (int)C, (int)P, (int)M, w);
    hipLaunchKernelGGL(bundle_scatter_points_kernel, dim3(mgrid), dim3(kThreads), 0, st, obs, (int)M, w);
    hipLaunchKernelGGL(bundle_sort_runs_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, w);
    if (tiles > 0) {
        hipLaunchKernelGGL(bundle_tile_count_kernel, dim3(tiles), dim3(kTile), 0, st, obs, (int)M, (int)C, tiles, w);
        hipLaunchKernelGGL(bundle_tile_scan_kernel, dim3(1), dim3(kSolveThreads), 0, st, (int)C, tiles, w);
        hipLaunchKernelGGL(bundle_tile_scatter_kernel, dim3(tiles), dim3(kTile), 0, st, obs, (int)M, (int)C, tiles, w);
    }
    hipLaunchKernelGGL(bundle_linearize_kernel, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, mask, poses_out,
                       points_out, (int)C, w);
    hipLaunchKernelGGL(bundle_camera_kernel, dim3((unsigned)C), dim3(kThreads), 0, st, obs, cam, mask, poses_out, points_out, w);
    hipLaunchKernelGGL(bundle_start_kernel, dim3(1), dim3(kThreads), 0, st, pblocks, mask, (int)C, max_steps, poses_out, w);
    for (int step = 0; step < max_steps; ++step) {
        hipLaunchKernelGGL(bundle_linearize_kernel, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, mask, poses_out,
                           points_out, (int)C, w);
        hipLaunchKernelGGL(bundle_camera_kernel, dim3((unsigned)C), dim3(kThreads), 0, st, obs, cam, mask, poses_out,
                           points_out, w);
        hipLaunchKernelGGL(bundle_point_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, w);
        if (pairs > 0) hipLaunchKernelGGL(bundle_schur_kernel, dim3(pairs), dim3(kThreads), 0, st, mask, (int)C, w);
        if (F <= kLdsFree)
            hipLaunchKernelGGL(bundle_solve_kernel<true>, dim3(1), dim3(kSolveThreads), 0, st, mask, (int)C, poses_out, w);
        else
            hipLaunchKernelGGL(bundle_solve_kernel<false>, dim3(1), dim3(kSolveThreads), 0, st, mask, (int)C, poses_out, w);
        hipLaunchKernelGGL(bundle_trial_kernel, dim3(pgrid), dim3(kThreads), 0, st, obs, (int)P, cam, mask, points_out, (int)C, w);
        hipLaunchKernelGGL(bundle_decide_kernel, dim3(1), dim3(kThreads), 0, st, pblocks, mask, (int)C, max_steps, poses_out, w);
        hipLaunchKernelGGL(bundle_commit_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, mask, (int)C, poses_out,
                           points_out, w);
    }
    hipLaunchKernelGGL(bundle_finish_kernel, dim3(1), dim3(1), 0, st, w, info);
    return check_launch("sfm_bundle_adjust");
}

}  // extern "C"
