// Rotation averaging over a view graph (the NumPy definition, operation by operation, is
// tests/rotation_averaging_oracle.py): one absolute rotation per camera that agrees with the relative rotations of all
// edges at once, by iteratively reweighted Gauss-Newton on the weighted graph Laplacian, each step solved by conjugate
// gradients with the Jacobi preconditioner.  fp64 throughout; off unless asked for.
//
// Set-up, once per call:
//   rotavg_init_kernel       the state, the order's counters, levels, the start rotations, which edges are active
//   rotavg_self_kernel       thread per edge: a self-pair sets the bad flag
//   sfmorder::launch_point_order   the 2Q half-edges (2q -> i_q, 2q + 1 -> j_q) grouped by camera, in increasing
//                            half-edge index inside a camera: the "observations" are the half-edges, the "points" the cameras
//   rotavg_level_kernel      round k, thread per camera: level k (and the tree rotation) from the cameras of level < k
//   rotavg_register_kernel   thread per camera / edge: registered, NaN for an unregistered camera, which edges are used
//   rotavg_adjacency_kernel  thread per half-edge position: the camera at the other end of a used edge, -1 otherwise
//   rotavg_start_kernel      one thread: the status of a call without steps
// Then per step, every launch reading the state first and returning at once after a stop:
//   rotavg_edge_kernel<false>  thread per edge: r = log(R_j^T (R_q R_i)), omega = w rho'(|r|^2), the cost per block
//   rotavg_system_kernel     thread per camera: d_c = sum omega, b_c = sum s omega r over its half-edges in order
//   rotavg_cg_init_kernel    one workgroup: the cost, x = 0, r = b, z = r / d, p = z
//   per CG iteration, each over at most kCgBlocks blocks that leave one partial sum each:
//                            rotavg_cg_apply_kernel     (q_c = sum omega (p_c - p_other) in half-edge order, p . q)
//                            rotavg_cg_update_kernel    (alpha, x, r, z = r / d, r.z and r.r)
//                            rotavg_cg_direction_kernel (rho, beta, p and the stop of CG)
//   rotavg_step_kernel       thread per camera: R_c <- R_c exp([x_c]x), the largest |x_c|_inf
//   rotavg_decide_kernel     one thread: the counters, CONVERGED / MAX_STEPS / CG_FAILED
// and at the end rotavg_edge_kernel<true> (the residuals and the final cost) and rotavg_finish_kernel (info, the filler).
// The host reads three flags (stop, CG done, the last level round that set something) from pinned memory once per batch of
// kRoundBatch level rounds, once per step and once per chunk of kCgChunk CG iterations, and enqueues no more work after a
// stop.  The device state alone decides the result.  No floating-point atomics and no memset nodes: every floating-point sum
// runs in an order fixed by the edge list alone, so a call is bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_loss.h"
#include "sfm_math.h"
#include "sfm_obs_order.h"
#include "sfm_pnp.h"
#include "sfm_so3.h"

namespace {

using sfm::block_sum;
using sfmhost::check_launch;
using sfmhost::fail;

constexpr int kThreads = 256;
constexpr int kOneGroup = 1024;    // the one-workgroup kernels
constexpr int kCgChunk = 10;       // CG iterations enqueued between two reads of the flags
constexpr int kCgBlocks = 1024;    // the most blocks of a CG launch: every block sums their partials again
constexpr int kRoundBatch = 32;    // level rounds enqueued between two reads of the flags

static_assert(sizeof(sfm_rotavg_info) == 40, "sfm_rotavg_info layout is part of the ABI");
static_assert(sizeof(sfm_rotavg_options) == 40, "sfm_rotavg_options layout is part of the ABI");

// Written by one thread of a launch (last_round, registered, unknowns and xmax_bits: by integer atomics or by stores of one
// value), read by every launch after it.
struct State {
    int32_t stop, cg_done, last_round;   // the host reads these three at once
    int32_t bad;                         // an index out of range or a self-pair
    int32_t cg_fail, cg_k, cg_total, cg_max;
    int32_t steps, status, unknowns, registered;
    int32_t have_initial, pad;
    unsigned long long xmax_bits;        // the largest |x_c|_inf of this step, as the bits of a non-negative double
    double rho[2];                       // r.z of CG iteration k in slot k & 1
    double tol2, cost, initial_cost;
};

struct Ws {
    State* st;
    sfmorder::PointOrder po;             // off [C + 1], fill [C], ord [2Q], tile_sum
    int32_t* level;                      // [C], -1 without a level
    uint8_t* used;                       // [Q]: 1 active, 2 active with both ends registered
    double *omega, *rvec;                // [Q], [3Q]
    int32_t* adj_other;                  // [2Q] per adjacency position: the camera at the other end of a used edge, else -1
    double* adj_omega;                   // [2Q] per adjacency position: omega of its edge in this step (used edges only)
    double *d, *b, *x, *r, *z, *p, *q;   // [C], [3C] each; 0 outside the free cameras
    double *part_pq, *part_rz;           // [kCgBlocks], [2 kCgBlocks]: the per-block shares of p.q, and of r.z and r.r
    double* cost_part;                   // [blocks(Q)]: the cost per block of edges
};

int64_t carve(uintptr_t base, int64_t C, int64_t Q, Ws* w) {
    sfmhost::Carver k{base, 0};
    w->st = k.take<State>(1);
    int32_t* off = k.take<int32_t>(C + 1);
    int32_t* fill = k.take<int32_t>(C);
    int32_t* ord = k.take<int32_t>(2 * Q);
    w->po = sfmorder::PointOrder{off, fill, ord, k.take<int32_t>(sfmorder::tiles(C)), nullptr};
    w->po.flag = base ? &w->st->bad : nullptr;
    w->level = k.take<int32_t>(C);
    w->used = k.take<uint8_t>(Q);
    w->omega = k.take<double>(Q);
    w->rvec = k.take<double>(3 * Q);
    w->adj_other = k.take<int32_t>(2 * Q);
    w->adj_omega = k.take<double>(2 * Q);
    w->d = k.take<double>(C);
    w->b = k.take<double>(3 * C);
    w->x = k.take<double>(3 * C);
    w->r = k.take<double>(3 * C);
    w->z = k.take<double>(3 * C);
    w->p = k.take<double>(3 * C);
    w->q = k.take<double>(3 * C);
    w->part_pq = k.take<double>(kCgBlocks);
    w->part_rz = k.take<double>(2 * kCgBlocks);
    w->cost_part = k.take<double>((Q + kThreads - 1) / kThreads);
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

__global__ __launch_bounds__(kThreads) void rotavg_self_kernel(Args a, Ws w) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q < a.Q && a.pairs[2 * q] == a.pairs[2 * q + 1]) w.st->bad = 1;   // every offender stores the same value
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

// Round k, thread per camera without a level: among its half-edges, in order, whose edge is active and whose other end has a
// level < k (set by an earlier launch: a level being written by this one reads as -1 or k), the heaviest edge, the first of
// equals.  It takes level k and, kTree, the rotation through that edge.  Round k - 1 having set nothing ends the rounds.
template <bool kTree>
__global__ __launch_bounds__(kThreads) void rotavg_level_kernel(int k, Args a, Ws w) {
    if (w.st->bad || w.st->last_round < k - 1) return;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= a.C || w.level[c] >= 0) return;
    int best = -1;
    double best_w = 0.0;
    for (int i = w.po.off[c]; i < w.po.off[c + 1]; ++i) {
        const int h = w.po.ord[i], q = h >> 1;
        if (!w.used[q]) continue;
        const int lv = w.level[a.pairs[h ^ 1]];
        if (lv < 0 || lv >= k) continue;
        const double wq = a.weights[q];
        if (best < 0 || wq > best_w) {
            best = h;
            best_w = wq;
        }
    }
    if (best < 0) return;
    w.level[c] = k;
    w.st->last_round = k;   // every camera of this round stores the same value
    if (!kTree) return;
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

// Thread i: camera i's registration (NaN rotation without a level; the free cameras counted); edge i used iff both ends are
__global__ __launch_bounds__(kThreads) void rotavg_register_kernel(Args a, Ws w) {
    if (w.st->bad) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.C) {
        const int lv = w.level[i];
        a.registered[i] = lv >= 0;
        if (a.level) a.level[i] = lv;
        if (lv < 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.R[9 * i + k] = (double)NAN;
        } else {
            atomicAdd(&w.st->registered, 1);
            if (i != a.root) atomicAdd(&w.st->unknowns, 1);
        }
    }
    if (i < a.Q && w.used[i] && w.level[a.pairs[2 * i]] >= 0 && w.level[a.pairs[2 * i + 1]] >= 0) w.used[i] = 2;
}

// Thread per adjacency position, after the registration: the other end of a used edge, -1 for a half-edge the sums skip
__global__ __launch_bounds__(kThreads) void rotavg_adjacency_kernel(Args a, Ws w) {
    if (w.st->bad) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= 2 * (int64_t)a.Q) return;
    const int h = w.po.ord[i];
    w.adj_other[i] = w.used[h >> 1] == 2 ? a.pairs[h ^ 1] : -1;
}

__global__ void rotavg_start_kernel(int max_steps, Ws w) {
    State* st = w.st;
    if (st->bad) {
        st->stop = 1;
        st->status = SFM_ROTAVG_BAD_INDEX;
    } else if (st->unknowns == 0) {
        st->stop = 1;
        st->status = SFM_ROTAVG_CONVERGED;
    } else if (max_steps == 0) {
        st->stop = 1;
        st->status = SFM_ROTAVG_MAX_STEPS;
    }
}

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

SFM_DEVICE bool is_free(const Args& a, const Ws& w, int c) { return c != a.root && w.level[c] >= 0; }

// Thread per camera: d_c = sum omega, b_c = sum s omega r over its used half-edges in order (0 for a camera that is not free);
// omega of every used half-edge of a free camera to its adjacency position
__global__ __launch_bounds__(kThreads) void rotavg_system_kernel(Args a, Ws w) {
    if (w.st->stop) return;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= a.C) return;
    double d = 0.0, b[3] = {0.0, 0.0, 0.0};
    if (is_free(a, w, c))
        for (int i = w.po.off[c]; i < w.po.off[c + 1]; ++i) {
            if (w.adj_other[i] < 0) continue;
            const int h = w.po.ord[i], q = h >> 1;
            const double om = w.omega[q], s = (h & 1) ? 1.0 : -1.0;
            w.adj_omega[i] = om;   // the CG passes read it in place of (ord, used, omega)
            d += om;
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k] += s * (om * w.rvec[3 * (int64_t)q + k]);
        }
    w.d[c] = d;
#pragma unroll
    for (int k = 0; k < 3; ++k) w.b[3 * (int64_t)c + k] = b[k];
}

// The sum of the per-block costs in a fixed order
template <int kBlock>
SFM_DEVICE double sum_cost(const Ws& w, int blocks, double* part, double* total) {
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < blocks; i += kBlock) v[0] += w.cost_part[i];
    block_sum<1, kBlock>(v, part, total);
    return total[0];
}

// One workgroup: the cost of this linearisation; x = 0, r = b, z = r / d, p = z, rho = r.z, tol2 = tol^2 |b|^2.  A non-finite
// rho or |b|^2 fails the step.  Sets cg_fail and cg_done afresh on every step that runs.
__global__ __launch_bounds__(kOneGroup) void rotavg_cg_init_kernel(Args a, int blocks, double tol, Ws w) {
    __shared__ double part[kOneGroup / kWave * 2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->stop) return;
    const double cost = sum_cost<kOneGroup>(w, blocks, part, total);
    double v[2] = {0.0, 0.0};   // r.z | b.b
    for (int c = threadIdx.x; c < a.C; c += kOneGroup) {
        const bool free_c = is_free(a, w, c);
        const double d = w.d[c];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t at = 3 * (int64_t)c + k;
            const double b = w.b[at], z = free_c ? b / d : 0.0;
            w.x[at] = 0.0;
            w.r[at] = b;
            w.z[at] = z;
            w.p[at] = z;
            v[0] += b * z;
            v[1] += b * b;
        }
    }
    block_sum<2, kOneGroup>(v, part, total);
    if (threadIdx.x != 0) return;
    const bool bad = !isfinite(total[0]) || !isfinite(total[1]);
    st->cost = cost;
    if (!st->have_initial) {
        st->have_initial = 1;
        st->initial_cost = cost;
    }
    st->cg_k = 0;
    st->rho[0] = total[0];
    st->tol2 = tol * tol * total[1];
    st->cg_fail = bad;
    st->cg_done = bad || total[1] <= st->tol2;
}

// The sum of n per-block partials of K doubles each in a fixed order: strided per thread, then block_sum.  Every block of a CG
// kernel sums the partials of the launch before it again (at most kCgBlocks of them) and so holds the same scalar.
template <int K>
SFM_DEVICE void sum_parts(const double* parts, int n, double* lds_part, double* total) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += parts[K * i + k];
    block_sum<K, kThreads>(v, lds_part, total);
}

// The three launches of CG iteration k (k comes from the host, which numbers the iterations it enqueues).  Each walks the
// cameras with a grid-stride loop over at most kCgBlocks blocks and leaves one partial per block; none of them changes a
// word of the state that a block of the same launch still reads, except cg_done going to 1, after which no block's work
// matters: rho alternates between two slots, and the counters are stored, not incremented.
//
// 1. q_c = sum over its used half-edges in order of omega (p_c - p_other); the block's share of p . q
__global__ __launch_bounds__(kThreads) void rotavg_cg_apply_kernel(Args a, Ws w) {
    __shared__ double part[kThreads / kWave];
    __shared__ double total[1];
    if (w.st->stop || w.st->cg_done) return;
    double pq[1] = {0.0};
    for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < a.C; c += (int64_t)gridDim.x * kThreads) {
        double acc[3] = {0.0, 0.0, 0.0};
        if (is_free(a, w, (int)c)) {
            const double pc[3] = {w.p[3 * c], w.p[3 * c + 1], w.p[3 * c + 2]};
            for (int i = w.po.off[c]; i < w.po.off[c + 1]; ++i) {
                const int o = w.adj_other[i];
                if (o < 0) continue;
                const double om = w.adj_omega[i];
                const double* po = w.p + 3 * (int64_t)o;
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[k] += om * (pc[k] - po[k]);
            }
            pq[0] += (pc[0] * acc[0] + pc[1] * acc[1]) + pc[2] * acc[2];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) w.q[3 * c + k] = acc[k];
    }
    block_sum<1, kThreads>(pq, part, total);
    if (threadIdx.x == 0) w.part_pq[blockIdx.x] = total[0];
}

// 2. alpha = rho / p.q, x += alpha p, r -= alpha q, z = r / d; the block's shares of r.z and r.r.  A breakdown (p.q <= 0 or a
// non-finite scalar) ends CG with the iterate reached so far; at k = 0, or with a non-finite scalar, it fails the call.
__global__ __launch_bounds__(kThreads) void rotavg_cg_update_kernel(Args a, int k, Ws w) {
    __shared__ double part[kThreads / kWave * 2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->stop || st->cg_done) return;
    const double rho = st->rho[k & 1];
    sum_parts<1>(w.part_pq, gridDim.x, part, total);
    const double pq = total[0];
    const double alpha = rho / pq;
    if (!(pq > 0.0) || !isfinite(pq) || !isfinite(alpha)) {   // every block finds the same
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->cg_done = 1;
            if (k == 0 || !isfinite(pq) || !isfinite(alpha)) st->cg_fail = 1;
        }
        return;
    }
    double v[2] = {0.0, 0.0};   // r.z | r.r
    for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < a.C; c += (int64_t)gridDim.x * kThreads) {
        const bool free_c = is_free(a, w, (int)c);
        const double d = w.d[c];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int64_t at = 3 * c + i;
            w.x[at] = w.x[at] + alpha * w.p[at];
            const double r = w.r[at] - alpha * w.q[at];
            const double z = free_c ? r / d : 0.0;
            w.r[at] = r;
            w.z[at] = z;
            v[0] += r * z;
            v[1] += r * r;
        }
    }
    block_sum<2, kThreads>(v, part, total);
    if (threadIdx.x < 2) w.part_rz[2 * blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

// 3. rho' = r.z, beta = rho' / rho, p = z + beta p.  CG stops at |r|^2 <= tol2, at max_iterations, or at a non-finite scalar
// (which fails the call); block 0 records it, the number of iterations done and rho' for iteration k + 1.
__global__ __launch_bounds__(kThreads) void rotavg_cg_direction_kernel(Args a, int k, int max_iterations, Ws w) {
    __shared__ double part[kThreads / kWave * 2];
    __shared__ double total[2];
    State* st = w.st;
    if (st->stop || st->cg_done) return;
    const double rho = st->rho[k & 1], tol2 = st->tol2;
    sum_parts<2>(w.part_rz, gridDim.x, part, total);
    const double rz = total[0], rr = total[1];
    const bool broke = !isfinite(rz) || !isfinite(rr);
    const double beta = rz / rho;
    const bool done = broke || rr <= tol2 || k + 1 == max_iterations;
    if (!done)
        for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < a.C; c += (int64_t)gridDim.x * kThreads)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int64_t at = 3 * c + i;
                w.p[at] = w.z[at] + beta * w.p[at];
            }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->cg_k = k + 1;
        st->rho[(k + 1) & 1] = rz;
        st->cg_done = done;
        if (broke) st->cg_fail = 1;
    }
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
    const double m = fmax(fmax(fabs(x[0]), fabs(x[1])), fabs(x[2]));
    // a NaN step reads as larger than every tolerance
    atomicMax(&w.st->xmax_bits, m == m ? (unsigned long long)__double_as_longlong(m) : 0x7FF8000000000000ull);
}

__global__ void rotavg_decide_kernel(int max_steps, double step_tolerance, Ws w) {
    State* st = w.st;
    if (st->stop) return;
    if (st->cg_fail) {
        st->stop = 1;
        st->status = SFM_ROTAVG_CG_FAILED;
        return;
    }
    const double xmax = __longlong_as_double((long long)st->xmax_bits);
    st->xmax_bits = 0;
    st->steps += 1;
    st->cg_total += st->cg_k;
    st->cg_max = max(st->cg_max, st->cg_k);
    if (xmax <= step_tolerance) {
        st->stop = 1;
        st->status = SFM_ROTAVG_CONVERGED;
    } else if (st->steps == max_steps) {
        st->stop = 1;
        st->status = SFM_ROTAVG_MAX_STEPS;
    }
}

// One workgroup, after the final edge pass: info; after a bad index the filler of every output.
__global__ __launch_bounds__(kOneGroup) void rotavg_finish_kernel(Args a, int blocks, Ws w, sfm_rotavg_info* __restrict__ info) {
    __shared__ double part[kOneGroup / kWave];
    __shared__ double total[1];
    const State* st = w.st;
    if (st->bad) {
        for (int64_t i = threadIdx.x; i < 9 * (int64_t)a.C; i += kOneGroup) a.R[i] = (double)NAN;
        for (int64_t i = threadIdx.x; i < a.C; i += kOneGroup) a.registered[i] = 0;
        for (int64_t i = threadIdx.x; a.level && i < a.C; i += kOneGroup) a.level[i] = -1;
        for (int64_t i = threadIdx.x; i < a.Q; i += kOneGroup) a.residual[i] = (double)NAN;
        if (threadIdx.x == 0)
            *info = sfm_rotavg_info{(double)NAN, (double)NAN, 0, SFM_ROTAVG_BAD_INDEX, 0, 0, 0, 0};
        return;
    }
    const double cost = sum_cost<kOneGroup>(w, blocks, part, total);
    if (threadIdx.x != 0) return;
    *info = sfm_rotavg_info{st->have_initial ? st->initial_cost : cost, cost, st->steps, st->status, st->cg_total, st->cg_max,
                            st->registered, st->last_round};
}

// The host's copy of the three flags {stop, cg_done, last_round}: pinned, one per host thread, allocated on its first call.
int32_t* pinned_flags() {
    thread_local int32_t* flags = nullptr;
    if (!flags && hipHostMalloc(reinterpret_cast<void**>(&flags), 3 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
        flags = nullptr;
    return flags;
}

int enqueue(const Args& a, const sfm_rotavg_options& o, const sfmloss::Loss& loss, const Ws& w, sfm_rotavg_info* info,
            int32_t* flags, hipStream_t st) {
    const int64_t C = a.C, Q = a.Q;
    const unsigned cgrid = sfmhost::grid_for(C, kThreads), qgrid = sfmhost::grid_for(Q, kThreads);
    const unsigned igrid = sfmhost::grid_for(C + 1 > Q ? C + 1 : Q, kThreads);
    const unsigned cg_grid = sfmhost::grid_stride(C, kThreads, kCgBlocks);
    const int qblocks = (int)((Q + kThreads - 1) / kThreads);
    auto read_flags = [&]() -> int {
        if (hipMemcpyAsync(flags, &w.st->stop, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return check_launch("sfm_average_rotations: read the flags");
        return SFM_OK;
    };
    hipLaunchKernelGGL(rotavg_init_kernel, dim3(igrid), dim3(kThreads), 0, st, a, w);
    if (Q > 0) hipLaunchKernelGGL(rotavg_self_kernel, dim3(qgrid), dim3(kThreads), 0, st, a, w);
    sfmorder::launch_point_order(a.pairs, a.pairs, 2 * Q, C, C, w.po, st);
    for (int k0 = 1; k0 < C; k0 += kRoundBatch) {
        int k = k0;
        for (; k < C && k < k0 + kRoundBatch; ++k) {
            if (a.given)
                hipLaunchKernelGGL(rotavg_level_kernel<false>, dim3(cgrid), dim3(kThreads), 0, st, k, a, w);
            else
                hipLaunchKernelGGL(rotavg_level_kernel<true>, dim3(cgrid), dim3(kThreads), 0, st, k, a, w);
        }
        if (k >= C) break;   // the last possible round is enqueued
        const int rc = read_flags();
        if (rc != SFM_OK) return rc;
        if (flags[2] < k - 1) break;   // a round set nothing (or the order refused an index)
    }
    hipLaunchKernelGGL(rotavg_register_kernel, dim3(igrid), dim3(kThreads), 0, st, a, w);
    if (Q > 0) hipLaunchKernelGGL(rotavg_adjacency_kernel, dim3(sfmhost::grid_for(2 * Q, kThreads)), dim3(kThreads), 0, st, a, w);
    hipLaunchKernelGGL(rotavg_start_kernel, dim3(1), dim3(1), 0, st, o.max_steps, w);
    for (int step = 0; step < o.max_steps; ++step) {
        int rc = read_flags();
        if (rc != SFM_OK) return rc;
        if (flags[0]) break;
        hipLaunchKernelGGL(rotavg_edge_kernel<false>, dim3(qgrid), dim3(kThreads), 0, st, a, loss, w);
        hipLaunchKernelGGL(rotavg_system_kernel, dim3(cgrid), dim3(kThreads), 0, st, a, w);
        hipLaunchKernelGGL(rotavg_cg_init_kernel, dim3(1), dim3(kOneGroup), 0, st, a, qblocks, o.cg_tolerance, w);
        for (int k0 = 0; k0 < o.max_cg_iterations; k0 += kCgChunk) {
            if (k0 > 0) {
                rc = read_flags();
                if (rc != SFM_OK) return rc;
                if (flags[0] || flags[1]) break;
            }
            for (int k = k0; k < o.max_cg_iterations && k < k0 + kCgChunk; ++k) {
                hipLaunchKernelGGL(rotavg_cg_apply_kernel, dim3(cg_grid), dim3(kThreads), 0, st, a, w);
                hipLaunchKernelGGL(rotavg_cg_update_kernel, dim3(cg_grid), dim3(kThreads), 0, st, a, k, w);
                hipLaunchKernelGGL(rotavg_cg_direction_kernel, dim3(cg_grid), dim3(kThreads), 0, st, a, k, o.max_cg_iterations, w);
            }
        }
        hipLaunchKernelGGL(rotavg_step_kernel, dim3(cgrid), dim3(kThreads), 0, st, a, w);
        hipLaunchKernelGGL(rotavg_decide_kernel, dim3(1), dim3(1), 0, st, o.max_steps, o.step_tolerance, w);
    }
    hipLaunchKernelGGL(rotavg_edge_kernel<true>, dim3(qgrid), dim3(kThreads), 0, st, a, loss, w);
    hipLaunchKernelGGL(rotavg_finish_kernel, dim3(1), dim3(kOneGroup), 0, st, a, qblocks, w, info);
    return check_launch("sfm_average_rotations");
}

bool sizes_ok(int64_t cameras, int64_t edges) {
    return cameras >= 1 && cameras < ((int64_t)1 << 31) && edges >= 0 && edges < ((int64_t)1 << 30);
}

}  // namespace

extern "C" {

int64_t sfm_average_rotations_workspace_bytes(int64_t cameras, int64_t edges) {
    if (!sizes_ok(cameras, edges)) return -1;
    Ws w;
    return carve(0, cameras, edges, &w);
}

int sfm_average_rotations(int64_t cameras, int64_t edges, const int32_t* pairs, const double* relative,
                          const double* weights, int64_t root, const double* initial, const sfm_rotavg_options* options,
                          double* rotations, uint8_t* registered, int32_t* level, double* residual, sfm_rotavg_info* info,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (!sizes_ok(cameras, edges))
        return fail(SFM_EINVAL, "sfm_average_rotations: cameras must be in [1, 2^31) and edges in [0, 2^30)");
    if (root < 0 || root >= cameras) return fail(SFM_EINVAL, "sfm_average_rotations: root must be a camera index");
    if (!options) return fail(SFM_EINVAL, "sfm_average_rotations: null pointer (options)");
    const sfm_rotavg_options o = *options;
    if (o.loss < SFM_BUNDLE_LOSS_SQUARED || o.loss > SFM_BUNDLE_LOSS_CAUCHY)
        return fail(SFM_EINVAL, "sfm_average_rotations: loss must be in 0..2");
    if (o.init != SFM_ROTAVG_INIT_TREE && o.init != SFM_ROTAVG_INIT_GIVEN)
        return fail(SFM_EINVAL, "sfm_average_rotations: init must be SFM_ROTAVG_INIT_TREE or SFM_ROTAVG_INIT_GIVEN");
    if (o.max_steps < 0) return fail(SFM_EINVAL, "sfm_average_rotations: max_steps must be at least 0");
    if (o.max_cg_iterations < 1) return fail(SFM_EINVAL, "sfm_average_rotations: max_cg_iterations must be at least 1");
    if (!(o.loss_scale > 0.0) || !isfinite(o.loss_scale))
        return fail(SFM_EINVAL, "sfm_average_rotations: loss_scale must be finite and positive");
    if (!(o.cg_tolerance > 0.0 && o.cg_tolerance < 1.0))
        return fail(SFM_EINVAL, "sfm_average_rotations: cg_tolerance must be finite and in (0, 1)");
    if (!(o.step_tolerance > 0.0) || !isfinite(o.step_tolerance))
        return fail(SFM_EINVAL, "sfm_average_rotations: step_tolerance must be finite and positive");
    const bool given = o.init == SFM_ROTAVG_INIT_GIVEN;
    if (!rotations || !registered || !info || !workspace || (given && !initial) ||
        (edges > 0 && (!pairs || !relative || !weights || !residual)))
        return fail(SFM_EINVAL, "sfm_average_rotations: null pointer");
    Ws w;
    if (workspace_bytes < carve((uintptr_t)workspace, cameras, edges, &w))
        return fail(SFM_EINVAL, "sfm_average_rotations: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_average_rotations: workspace must be 16-byte aligned");
    int32_t* flags = pinned_flags();
    if (!flags) return fail(SFM_EHIP, "sfm_average_rotations: no pinned host memory for the flags");
    const sfmloss::Loss loss{o.loss, 0, o.loss_scale, o.loss_scale * o.loss_scale};
    const Args a{(int)cameras, (int)edges, (int)root, given, pairs, relative, weights, initial, rotations, registered, level, residual};
    return enqueue(a, o, loss, w, info, flags, (hipStream_t)stream);
}

}  // extern "C"
