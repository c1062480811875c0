// What the two averaging solvers over a camera graph share (rotation averaging, DESIGN.md §6t, and translation averaging,
// §6u), defined once: the state and the workspace, the self-pair check, the level rounds with the tree start as a policy,
// registration, adjacency, the weighted graph Laplacian system, the three-launch conjugate-gradient iteration with the
// Jacobi preconditioner, the step maximum, the stop decision, the host loop that reads three flags from pinned memory, the
// checks of an entry point (check_entry) and the info record at the end of a finish kernel (finish_info).
//
// A solver brings an `Args` (a trivially copyable struct passed to every kernel by value) with
//   int C, Q, root;  const int32_t* pairs;  const double* weights;  uint8_t* registered;  int32_t* level;
//   SFM_DEVICE void clear_camera(int64_t c) const    the NaN filler of an unregistered camera's output
// a tree policy `Tree` with
//   static constexpr bool kOn;  static SFM_DEVICE void place(const Args&, int c, int best)   camera c through half-edge best
// and a `Driver` with the launches that are its own (init, edge, step, final; see run()).
// Per edge the solver's edge kernel stores a weight in Ws::omega and a 3-vector in Ws::rvec; the system is then
//   sum_{q at c} omega (x_c - x_other) = sum_{q at c} s omega rvec    (s = +1 at the j end, -1 at the i end; x_root = 0)
// with every sum over a camera's used half-edges in increasing half-edge index.  A free camera whose row is zero (every
// omega at it 0) gets the diagonal 1 and with its zero right-hand side a zero step.  No floating-point atomics and no
// memset nodes: every floating-point sum runs in an order fixed by the edge list alone.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "sfm_common.h"
#include "sfm_loss.h"
#include "sfm_math.h"
#include "sfm_obs_order.h"

namespace graphcg {

using sfm::block_sum;

constexpr int kThreads = 256;
constexpr int kOneGroup = 1024;    // the one-workgroup kernels
constexpr int kCgChunk = 10;       // CG iterations enqueued between two reads of the flags
constexpr int kCgBlocks = 1024;    // the most blocks of a CG launch: every block sums their partials again
constexpr int kRoundBatch = 32;    // level rounds enqueued between two reads of the flags

// the statuses of both solvers (SFM_ROTAVG_* and SFM_TRANSAVG_* carry these values)
constexpr int kConverged = 0, kMaxSteps = 1, kCgFailed = 2, kBadIndex = 3;
// the starts of both solvers (SFM_ROTAVG_INIT_* and SFM_TRANSAVG_INIT_*)
constexpr int kInitTree = 0, kInitGiven = 1;

// finish_info() writes either info record: one layout under two names
#define SFM_SAME_FIELD(f) (offsetof(sfm_rotavg_info, f) == offsetof(sfm_transavg_info, f))
static_assert(sizeof(sfm_rotavg_info) == sizeof(sfm_transavg_info) && SFM_SAME_FIELD(initial_cost) && SFM_SAME_FIELD(final_cost) &&
                  SFM_SAME_FIELD(steps) && SFM_SAME_FIELD(status) && SFM_SAME_FIELD(cg_iterations) && SFM_SAME_FIELD(cg_max) &&
                  SFM_SAME_FIELD(registered) && SFM_SAME_FIELD(rounds),
              "sfm_rotavg_info and sfm_transavg_info have one layout");
#undef SFM_SAME_FIELD

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

inline void carve(sfmhost::Carver& k, int64_t C, int64_t Q, Ws* w) {
    const uintptr_t base = k.base;
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
}

inline bool sizes_ok(int64_t cameras, int64_t edges) {
    return cameras >= 1 && cameras < ((int64_t)1 << 31) && edges >= 0 && edges < ((int64_t)1 << 30);
}

struct NoTree {
    static constexpr bool kOn = false;
    template <class Args>
    static SFM_DEVICE void place(const Args&, int, int) {}
};

template <class Args>
__global__ __launch_bounds__(kThreads) void self_kernel(Args a, Ws w) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q < a.Q && a.pairs[2 * q] == a.pairs[2 * q + 1]) w.st->bad = 1;   // every offender stores the same value
}

// Round k, thread per camera without a level: among its half-edges, in order, whose edge is active and whose other end has a
// level < k (set by an earlier launch: a level being written by this one reads as -1 or k), the heaviest edge, the first of
// equals.  It takes level k and, Tree::kOn, its start through that edge.  Round k - 1 having set nothing ends the rounds.
template <class Tree, class Args>
__global__ __launch_bounds__(kThreads) void level_kernel(int k, Args a, Ws w) {
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
    if (!Tree::kOn) return;
    Tree::place(a, c, best);
}

// Thread i: camera i's registration (the NaN filler without a level; the free cameras counted); edge i used iff both ends are
template <class Args>
__global__ __launch_bounds__(kThreads) void register_kernel(Args a, Ws w) {
    if (w.st->bad) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.C) {
        const int lv = w.level[i];
        a.registered[i] = lv >= 0;
        if (a.level) a.level[i] = lv;
        if (lv < 0) {
            a.clear_camera(i);
        } else {
            atomicAdd(&w.st->registered, 1);
            if (i != a.root) atomicAdd(&w.st->unknowns, 1);
        }
    }
    if (i < a.Q && w.used[i] && w.level[a.pairs[2 * i]] >= 0 && w.level[a.pairs[2 * i + 1]] >= 0) w.used[i] = 2;
}

// Thread per adjacency position, after the registration: the other end of a used edge, -1 for a half-edge the sums skip
template <class Args>
__global__ __launch_bounds__(kThreads) void adjacency_kernel(Args a, Ws w) {
    if (w.st->bad) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= 2 * (int64_t)a.Q) return;
    const int h = w.po.ord[i];
    w.adj_other[i] = w.used[h >> 1] == 2 ? a.pairs[h ^ 1] : -1;
}

static __global__ void start_kernel(int max_steps, Ws w) {
    State* st = w.st;
    if (st->bad) {
        st->stop = 1;
        st->status = kBadIndex;
    } else if (st->unknowns == 0) {
        st->stop = 1;
        st->status = kConverged;
    } else if (max_steps == 0) {
        st->stop = 1;
        st->status = kMaxSteps;
    }
}

template <class Args>
SFM_DEVICE bool is_free(const Args& a, const Ws& w, int c) { return c != a.root && w.level[c] >= 0; }

// Thread per camera: d_c = sum omega, b_c = sum s omega rvec over its used half-edges in order (0 for a camera that is not
// free); omega of every used half-edge of a free camera to its adjacency position.  A free camera with d_c = 0 gets d_c = 1.
template <class Args>
__global__ __launch_bounds__(kThreads) void system_kernel(Args a, Ws w) {
    if (w.st->stop) return;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= a.C) return;
    double d = 0.0, b[3] = {0.0, 0.0, 0.0};
    const bool free_c = is_free(a, w, c);
    if (free_c)
        for (int i = w.po.off[c]; i < w.po.off[c + 1]; ++i) {
            if (w.adj_other[i] < 0) continue;
            const int h = w.po.ord[i], q = h >> 1;
            const double om = w.omega[q], s = (h & 1) ? 1.0 : -1.0;
            w.adj_omega[i] = om;   // the CG passes read it in place of (ord, used, omega)
            d += om;
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k] += s * (om * w.rvec[3 * (int64_t)q + k]);
        }
    w.d[c] = free_c && d == 0.0 ? 1.0 : d;
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
template <class Args>
__global__ __launch_bounds__(kOneGroup) void cg_init_kernel(Args a, int blocks, double tol, Ws w) {
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
template <class Args>
__global__ __launch_bounds__(kThreads) void cg_apply_kernel(Args a, Ws w) {
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
template <class Args>
__global__ __launch_bounds__(kThreads) void cg_update_kernel(Args a, int k, Ws w) {
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
template <class Args>
__global__ __launch_bounds__(kThreads) void cg_direction_kernel(Args a, int k, int max_iterations, Ws w) {
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

// The largest |x_c|_inf of a step: an integer maximum over the bits of non-negative doubles; a NaN step reads as larger than
// every tolerance
SFM_DEVICE void record_step(const Ws& w, const double* x) {
    const double m = fmax(fmax(fabs(x[0]), fabs(x[1])), fabs(x[2]));
    atomicMax(&w.st->xmax_bits, m == m ? (unsigned long long)__double_as_longlong(m) : 0x7FF8000000000000ull);
}

// One thread, after the step kernel.  A step with index below min_converged_steps does not end the call as converged.
static __global__ void decide_kernel(int max_steps, int min_converged_steps, double step_tolerance, Ws w) {
    State* st = w.st;
    if (st->stop) return;
    if (st->cg_fail) {
        st->stop = 1;
        st->status = kCgFailed;
        return;
    }
    const double xmax = __longlong_as_double((long long)st->xmax_bits);
    st->xmax_bits = 0;
    st->steps += 1;
    st->cg_total += st->cg_k;
    st->cg_max = max(st->cg_max, st->cg_k);
    if (xmax <= step_tolerance && st->steps > min_converged_steps) {
        st->stop = 1;
        st->status = kConverged;
    } else if (st->steps == max_steps) {
        st->stop = 1;
        st->status = kMaxSteps;
    }
}

// The end of a solver's finish kernel (one workgroup of kOneGroup threads, after the final edge pass): after a bad index the
// filler of `registered` and `level` (the solver's kernel fills its own arrays with NaN) and the BAD_INDEX record; otherwise
// the final cost and the record from the state.
template <class Info, class Args>
SFM_DEVICE void finish_info(const Args& a, int blocks, const Ws& w, Info* __restrict__ info) {
    __shared__ double part[kOneGroup / kWave];
    __shared__ double total[1];
    const State* st = w.st;
    if (st->bad) {
        for (int64_t i = threadIdx.x; i < a.C; i += kOneGroup) a.registered[i] = 0;
        for (int64_t i = threadIdx.x; a.level && i < a.C; i += kOneGroup) a.level[i] = -1;
        if (threadIdx.x == 0) *info = Info{(double)NAN, (double)NAN, 0, kBadIndex, 0, 0, 0, 0};
        return;
    }
    const double cost = sum_cost<kOneGroup>(w, blocks, part, total);
    if (threadIdx.x != 0) return;
    *info = Info{st->have_initial ? st->initial_cost : cost, cost, st->steps, st->status, st->cg_total, st->cg_max,
                 st->registered, st->last_round};
}

// The host's copy of the three flags {stop, cg_done, last_round}: pinned, one per host thread, allocated on its first call.
inline int32_t* pinned_flags() {
    thread_local int32_t* flags = nullptr;
    if (!flags && hipHostMalloc(reinterpret_cast<void**>(&flags), 3 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
        flags = nullptr;
    return flags;
}

// Every check of an entry point before its first launch (a refused call has enqueued nothing), in the order of the texts
// below; the message is "<name>: <text>".  `o` is read only where `has_options`; `tag` names the solver's SFM_<tag>_INIT_*.
// `own`: the refusal of the solver's own option checks, whose place is after max_cg_iterations, or nullptr.  `pointers`: every
// pointer the call needs is there.  `needed`: the size of the workspace from the solver's carve (any value for refused
// sizes).  On SFM_OK *flags is the host's copy of the three flags.
template <class Options>
int check_entry(const char* name, const char* tag, int64_t cameras, int64_t edges, int64_t root, bool has_options,
                const Options& o, const char* own, bool pointers, const void* workspace, int64_t workspace_bytes,
                int64_t needed, int32_t** flags) {
    char init[80];
    snprintf(init, sizeof(init), "init must be SFM_%s_INIT_TREE or SFM_%s_INIT_GIVEN", tag, tag);
    const char* text =
        !sizes_ok(cameras, edges)                                  ? "cameras must be in [1, 2^31) and edges in [0, 2^30)"
        : root < 0 || root >= cameras                              ? "root must be a camera index"
        : !has_options                                             ? "null pointer (options)"
        : o.loss < SFM_BUNDLE_LOSS_SQUARED || o.loss > SFM_BUNDLE_LOSS_CAUCHY ? "loss must be in 0..2"
        : o.init != kInitTree && o.init != kInitGiven              ? init
        : o.max_steps < 0                                          ? "max_steps must be at least 0"
        : o.max_cg_iterations < 1                                  ? "max_cg_iterations must be at least 1"
        : own                                                      ? own
        : !sfmloss::scale_ok(o.loss_scale)                         ? "loss_scale must be positive with a normal finite square"
        : !(o.cg_tolerance > 0.0 && o.cg_tolerance < 1.0)          ? "cg_tolerance must be finite and in (0, 1)"
        : !(o.step_tolerance > 0.0) || !isfinite(o.step_tolerance) ? "step_tolerance must be finite and positive"
        : !pointers                                                ? "null pointer"
        : workspace_bytes < needed                                 ? "workspace too small"
        : ((uintptr_t)workspace & 15) != 0                         ? "workspace must be 16-byte aligned"
                                                                   : nullptr;
    int code = SFM_EINVAL;
    if (!text && !(*flags = pinned_flags())) {
        text = "no pinned host memory for the flags";
        code = SFM_EHIP;
    }
    if (!text) return SFM_OK;
    snprintf(sfmhost::error_buffer(), sfmhost::kErrorBytes, "%s: %s", name, text);
    return code;
}

struct Limits {
    int max_steps, max_cg_iterations, min_converged_steps;
    double cg_tolerance, step_tolerance;
};

// The launches of one call.  The host reads the flags once per batch of kRoundBatch level rounds, once per step and once per
// chunk of kCgChunk CG iterations, and enqueues no more work after a stop; the device state alone decides the result.
// `Driver` supplies what the solver owns:
//   init(igrid)            thread i: the state (thread 0), po.off[i] = 0, the level and the start of camera i, edge i active or not
//   tree_given()           true: the level rounds run with NoTree
//   edge(step, qgrid)      thread per edge: omega, rvec and the cost per block of the linearisation of step `step`
//   step(cgrid)            thread per camera: the update from w.x and record_step
//   finish(qgrid, qblocks) the final edge pass and the finish kernel
template <class Tree, class Args, class Driver>
int run(const Args& a, const Limits& o, const Ws& w, Driver& drv, int32_t* flags, hipStream_t st, const char* what) {
    const int64_t C = a.C, Q = a.Q;
    const unsigned cgrid = sfmhost::grid_for(C, kThreads), qgrid = sfmhost::grid_for(Q, kThreads);
    const unsigned igrid = sfmhost::grid_for(C + 1 > Q ? C + 1 : Q, kThreads);
    const unsigned cg_grid = sfmhost::grid_stride(C, kThreads, kCgBlocks);
    const int qblocks = (int)((Q + kThreads - 1) / kThreads);
    auto read_flags = [&]() -> int {
        if (hipMemcpyAsync(flags, &w.st->stop, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return sfmhost::check_launch(what);
        return SFM_OK;
    };
    drv.init(igrid);
    if (Q > 0) hipLaunchKernelGGL(self_kernel<Args>, dim3(qgrid), dim3(kThreads), 0, st, a, w);
    sfmorder::launch_point_order(a.pairs, a.pairs, 2 * Q, C, C, w.po, st);
    const bool given = drv.tree_given();
    for (int k0 = 1; k0 < C; k0 += kRoundBatch) {
        int k = k0;
        for (; k < C && k < k0 + kRoundBatch; ++k) {
            if (given)
                hipLaunchKernelGGL((level_kernel<NoTree, Args>), dim3(cgrid), dim3(kThreads), 0, st, k, a, w);
            else
                hipLaunchKernelGGL((level_kernel<Tree, Args>), dim3(cgrid), dim3(kThreads), 0, st, k, a, w);
        }
        if (k >= C) break;   // the last possible round is enqueued
        const int rc = read_flags();
        if (rc != SFM_OK) return rc;
        if (flags[2] < k - 1) break;   // a round set nothing (or the order refused an index)
    }
    hipLaunchKernelGGL(register_kernel<Args>, dim3(igrid), dim3(kThreads), 0, st, a, w);
    if (Q > 0) hipLaunchKernelGGL(adjacency_kernel<Args>, dim3(sfmhost::grid_for(2 * Q, kThreads)), dim3(kThreads), 0, st, a, w);
    hipLaunchKernelGGL(start_kernel, dim3(1), dim3(1), 0, st, o.max_steps, w);
    for (int step = 0; step < o.max_steps; ++step) {
        int rc = read_flags();
        if (rc != SFM_OK) return rc;
        if (flags[0]) break;
        drv.edge(step, qgrid);
        hipLaunchKernelGGL(system_kernel<Args>, dim3(cgrid), dim3(kThreads), 0, st, a, w);
        hipLaunchKernelGGL(cg_init_kernel<Args>, dim3(1), dim3(kOneGroup), 0, st, a, qblocks, o.cg_tolerance, w);
        for (int k0 = 0; k0 < o.max_cg_iterations; k0 += kCgChunk) {
            if (k0 > 0) {
                rc = read_flags();
                if (rc != SFM_OK) return rc;
                if (flags[0] || flags[1]) break;
            }
            for (int k = k0; k < o.max_cg_iterations && k < k0 + kCgChunk; ++k) {
                hipLaunchKernelGGL(cg_apply_kernel<Args>, dim3(cg_grid), dim3(kThreads), 0, st, a, w);
                hipLaunchKernelGGL(cg_update_kernel<Args>, dim3(cg_grid), dim3(kThreads), 0, st, a, k, w);
                hipLaunchKernelGGL(cg_direction_kernel<Args>, dim3(cg_grid), dim3(kThreads), 0, st, a, k, o.max_cg_iterations, w);
            }
        }
        drv.step(cgrid);
        hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(1), 0, st, o.max_steps, o.min_converged_steps, o.step_tolerance, w);
    }
    drv.finish(qgrid, qblocks);
    return sfmhost::check_launch(what);
}

}  // namespace graphcg
