// What every Levenberg-Marquardt loop of the library shares: the constants, the step rules and the
// Cholesky factor, solve and inverse of a small dense SPD matrix.  The sites are the two bundle adjusters
// (sfm_bundle_lm.h, sfm_bundle_pcg.hip), the refinement of the PnP winner (sfm_pnp_refine.hip), that of every pair's
// relative pose (sfm_view_graph_refine.hip) and the per-point refinement of sfm_tracks.hip.  Each site keeps its own loop
// and the order in which it asks the rules: the bundle adjusters know the points' share of |delta| only after the trial
// and test the small step there, the other three test it before the trial.  The NumPy oracles under tests/ keep constants and loops of their own: the independent definition.
// Not here, on purpose: cholesky3 of sfm_tracks.hip (another subtraction order, pinned by its oracle) and the
// conjugate-gradient loops of sfm_bundle_pcg.hip and sfm_graph_cg.h.
#pragma once
#include <math.h>

#include "sfm_math.h"

namespace sfmlm {

constexpr double kLambda0 = 1e-3;
constexpr double kLambdaMax = 1e16;
constexpr double kMinDecrease = 1e-12;  // stop when an accepted step lowers C by less than this fraction of C
constexpr double kMinStep = 1e-12;      // stop when |delta| <= kMinStep * (1 + |x|), x what the step moves
// The undamped H of a start point must have full rank: every Cholesky pivot above this fraction of its diagonal entry.
// Inliers that pin fewer degrees of freedom than the unknown has (all at one 3-D point, say) stop the round.
constexpr double kRankFloor = 1e-10;

// ---- The step rules ----------------------------------------------------------------------------------------------------
// No further trial: the step budget is spent, or the damping has left its range.
SFM_DEVICE bool exhausted(int steps, int max_steps, double lambda) { return steps >= max_steps || lambda > kLambdaMax; }

// The step is too short to matter: dn = |delta|, xn = |x|.
SFM_DEVICE bool small_step(double dn, double xn) { return dn <= kMinStep * (1.0 + xn); }

// The trial is accepted: a finite cost below the current one (a NaN or infinite trial cost never is).
SFM_DEVICE bool improved(double c_new, double c_old) { return isfinite(c_new) && c_new < c_old; }

// An accepted trial that lowered the cost by less than kMinDecrease of it is the last one.
SFM_DEVICE bool converged(double c_old, double c_new) { return c_old - c_new < kMinDecrease * c_old; }

// lambda after a rejected or failed trial, and after an accepted one
SFM_DEVICE double more_damping(double lambda) { return lambda * 10.0; }
SFM_DEVICE double less_damping(double lambda) { return lambda / 10.0; }

// ---- Small dense SPD matrices, by one thread, in registers.  Damping (A[i][i] + lambda * A[i][i]) is the caller's ------
// The Cholesky factor L (lower triangle; the entries above the diagonal are left alone) of the symmetric A, column by
// column, every sum by sequential subtraction with k ascending: s = A[j][j]; s -= L[j][k] * L[j][k].  False when a pivot
// s is not above rel times its diagonal entry; L is completed all the same, with sqrt(max(s, 0)) on the diagonal.
// rel = 0 asks for a positive, finite pivot: `s > 0 * A[j][j]` is false for a NaN s, and also for s = +inf, because
// subtracting finite or NaN terms from A[j][j] gives +inf only if A[j][j] is +inf, and then 0 * inf is NaN.  A NaN
// diagonal entry makes s NaN.  So the one test equals `s > 0 && isfinite(s)`.
template <int N>
SFM_DEVICE bool factor(const double (&A)[N][N], double rel, double (&L)[N][N]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        ok = ok && s > rel * A[j][j];
        L[j][j] = sqrt(fmax(s, 0.0));
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double x = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) x -= L[i][k] * L[j][k];
            L[i][j] = x / L[j][j];
        }
    }
    return ok;
}

// x with L L^T x = b: forward, then back substitution.  False when an entry of x is not finite.
template <int N>
SFM_DEVICE bool solve(const double (&L)[N][N], const double (&b)[N], double (&x)[N]) {
    double y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double v = b[j];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= L[j][k] * y[k];
        y[j] = v / L[j][j];
    }
    bool finite = true;
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
        double v = y[j];
#pragma unroll
        for (int k = j + 1; k < N; ++k) v -= L[k][j] * x[k];
        x[j] = v / L[j][j];
        finite = finite && isfinite(x[j]);
    }
    return finite;
}

// inv = (L L^T)^-1 = L^-T L^-1, all N x N entries: the columns of L^-1 by forward substitution, then
// inv[i][j] = sum over k >= max(i, j) of Li[k][i] * Li[k][j], k ascending from that first non-zero term.
template <int N>
SFM_DEVICE void inverse(const double (&L)[N][N], double (&inv)[N][N]) {
    double Li[N][N];
#pragma unroll
    for (int c = 0; c < N; ++c)
#pragma unroll
        for (int i = c; i < N; ++i) {
            double x = i == c ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k) x -= L[i][k] * Li[k][c];
            Li[i][c] = x / L[i][i];
        }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < N; ++k) v += Li[k][i] * Li[k][j];
            inv[i][j] = inv[j][i] = v;
        }
}

}  // namespace sfmlm
