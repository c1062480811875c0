// Sub-pixel refinement of track observations by affine least-squares patch matching (definition:
// tests/track_refine_oracle.py).  Every observation of a track but the reference is aligned with the reference's window by
// Gauss-Newton on six affine parameters, maximising the normalised correlation.  All arithmetic is fp64 with + - * / and sqrt in
// the definition's order, so the device equals the NumPy definition byte for byte.  The bilinear cell formula is sfm_dense.h's.
//
//   refine_kernel<SPL>   one wave per observation, four observations per block.  Window sample k = lane + 64 j (j < SPL, SPL =
//                        ceil((2r+1)^2 / 64)) belongs to lane k mod 64; template, state and every running sum stay in registers.
//                        A sum over the window: each lane adds its samples with j ascending (a lane without a sample adds 0.0),
//                        then s += s[lane xor m] for m = 32, 16, 8, 4, 2, 1 -- every lane ends with the same bits.  The 6 x 6
//                        system is solved redundantly in every lane (sfmlm::factor / solve); lane 0 writes the outputs.
//                        No LDS, no barrier, no atomics; every exit is wave-uniform.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_dense.h"
#include "sfm_keypoint_planes.h"
#include "sfm_lm.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmplanes::CheckedTable;
using sfmplanes::DevPlane;

constexpr int kObsPerBlock = 4;
constexpr int kBlock = kObsPerBlock * kWave;
constexpr int kMaxRadius = 7, kMinRadius = 2, kMaxIterations = 50;

struct RefineArgs {
    const DevPlane* planes;
    const uint8_t* pool;
    const int32_t *plane, *x, *y, *reference;
    const double* warp0;
    double *xy, *warp, *correlation;
    int32_t *iterations, *status;
    int64_t M;
    int n_planes, radius, max_iterations;
    double min_step2, max_shift2, min_correlation;
};

// The sum of one value per lane, in every lane.  Not sfm::wave_sum: the order of this xor butterfly is section 6al's definition.
SFM_DEVICE double butterfly_sum(double v) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, kWave);
    return v;
}

template <int SPL>
SFM_DEVICE double window_sum(const double (&p)[SPL]) {
    double acc = p[0];
#pragma unroll
    for (int j = 1; j < SPL; ++j) acc = acc + p[j];
    return butterfly_sum(acc);
}

// section 6ai's bilinear formula (sfm_dense.h) at (u, v), 0 <= u <= W - 1 and 0 <= v <= H - 1; the cell is the last one of its
// row or column when u + 1 or v + 1 rounded up to the plane's edge
SFM_DEVICE double bilinear(const uint8_t* __restrict__ image, int W, int H, double u, double v) {
    const int x0 = min((int)u, W - 2), y0 = min((int)v, H - 2);
    return sfmdense::bilinear_cell(image + (int64_t)y0 * W + x0, W, u - (double)x0, v - (double)y0);
}

// The window's positions under (t, A); false when a sample leaves 1 <= u < W - 2, 1 <= v < H - 2 (wave-uniform).
template <int SPL>
SFM_DEVICE bool window_positions(const double (&dx)[SPL], const double (&dy)[SPL], const bool (&active)[SPL], double t0, double t1,
                                        const double (&A)[4], int W, int H, double (&u)[SPL], double (&v)[SPL]) {
    bool bad = false;
    const double ulim = (double)(W - 2), vlim = (double)(H - 2);
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        u[j] = t0 + (A[0] * dx[j] + A[1] * dy[j]);
        v[j] = t1 + (A[2] * dx[j] + A[3] * dy[j]);
        const bool inside = 1.0 <= u[j] && u[j] < ulim && 1.0 <= v[j] && v[j] < vlim;   // false for a NaN
        bad = bad || (active[j] && !inside);
    }
    return __ballot(bad) == 0ull;
}

// I0 = I - mean(I) in place (0 in a lane without the sample); returns the sum of I0^2
template <int SPL>
SFM_DEVICE double centre(double (&I)[SPL], const bool (&active)[SPL], double n) {
    const double mean = window_sum<SPL>(I) / n;
    double sq[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        I[j] = active[j] ? I[j] - mean : 0.0;
        sq[j] = I[j] * I[j];
    }
    return window_sum<SPL>(sq);
}

SFM_DEVICE void write_result(const RefineArgs& a, int64_t o, int lane, int status, double x, double y, const double (&A)[4],
                                    double correlation, int iterations) {
    if (lane != 0) return;
    a.xy[2 * o] = x;
    a.xy[2 * o + 1] = y;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.warp[4 * o + k] = A[k];
    a.correlation[o] = correlation;
    a.iterations[o] = iterations;
    a.status[o] = status;
}

template <int SPL>
__global__ __launch_bounds__(kBlock) void refine_kernel(RefineArgs a) {
    const int lane = (int)(threadIdx.x % kWave);
    const int64_t o = (int64_t)blockIdx.x * kObsPerBlock + (int64_t)(threadIdx.x / kWave);
    if (o >= a.M) return;
    const int xi = a.x[o], yi = a.y[o], po = a.plane[o], q = a.reference[o];
    double A0[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) A0[k] = a.warp0[4 * o + k];
    const double x0 = (double)xi, y0 = (double)yi;
    if (q == -1 || (int64_t)q == o) return write_result(a, o, lane, SFM_REFINE_REFERENCE, x0, y0, A0, NAN, 0);
    if (q < 0 || (int64_t)q >= a.M || po < 0 || po >= a.n_planes) return write_result(a, o, lane, SFM_REFINE_BAD_INDEX, x0, y0, A0, NAN, 0);
    const int xq = a.x[q], yq = a.y[q], pq = a.plane[q];
    if (pq < 0 || pq >= a.n_planes) return write_result(a, o, lane, SFM_REFINE_BAD_INDEX, x0, y0, A0, NAN, 0);
    const DevPlane plane_o = a.planes[po], plane_q = a.planes[pq];
    const int W = plane_o.width, H = plane_o.height, Wq = plane_q.width, Hq = plane_q.height;
    if (xi < 0 || xi >= W || yi < 0 || yi >= H || xq < 0 || xq >= Wq || yq < 0 || yq >= Hq)
        return write_result(a, o, lane, SFM_REFINE_BAD_INDEX, x0, y0, A0, NAN, 0);
    const int r = a.radius, side = 2 * r + 1, count = side * side;
    const double n = (double)count;
    if (xq - r < 0 || xq + r > Wq - 1 || yq - r < 0 || yq + r > Hq - 1)
        return write_result(a, o, lane, SFM_REFINE_OUTSIDE, x0, y0, A0, NAN, 0);

    // the window and the template
    bool active[SPL];
    double dx[SPL], dy[SPL], T[SPL];
    const uint8_t* __restrict__ ref_image = a.pool + plane_q.offset;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int k = lane + kWave * j;
        active[j] = k < count;
        const int row = k / side, col = k - row * side;
        dx[j] = (double)(col - r);
        dy[j] = (double)(row - r);
        T[j] = active[j] ? (double)ref_image[(int64_t)(yq + row - r) * Wq + (xq + col - r)] : 0.0;
    }
    {
        const double ss = centre<SPL>(T, active, n);
        if (ss == 0.0) return write_result(a, o, lane, SFM_REFINE_FLAT, x0, y0, A0, NAN, 0);
        const double norm = sqrt(ss);
#pragma unroll
        for (int j = 0; j < SPL; ++j) T[j] = T[j] / norm;
    }

    const uint8_t* __restrict__ image = a.pool + plane_o.offset;
    double t0 = x0, t1 = y0;
    double A[4] = {A0[0], A0[1], A0[2], A0[3]};
    int solves = 0;
    double u[SPL], v[SPL], I[SPL];
#pragma unroll 1
    for (int it = 0; it < a.max_iterations; ++it) {
        if (!window_positions<SPL>(dx, dy, active, t0, t1, A, W, H, u, v))
            return write_result(a, o, lane, SFM_REFINE_OUTSIDE, x0, y0, A0, NAN, solves);
        double gx[SPL], gy[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            I[j] = gx[j] = gy[j] = 0.0;
            if (active[j]) {
                I[j] = bilinear(image, W, H, u[j], v[j]);
                gx[j] = 0.5 * (bilinear(image, W, H, u[j] + 1.0, v[j]) - bilinear(image, W, H, u[j] - 1.0, v[j]));
                gy[j] = 0.5 * (bilinear(image, W, H, u[j], v[j] + 1.0) - bilinear(image, W, H, u[j], v[j] - 1.0));
            }
        }
        const double ss = centre<SPL>(I, active, n);
        if (ss == 0.0) return write_result(a, o, lane, SFM_REFINE_FLAT, x0, y0, A0, NAN, solves);
        const double s = sqrt(ss);
        double res[SPL], J[6][SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            res[j] = T[j] - I[j] / s;
            J[0][j] = gx[j] / s;
            J[1][j] = gy[j] / s;
            J[2][j] = gx[j] * dx[j] / s;
            J[3][j] = gx[j] * dy[j] / s;
            J[4][j] = gy[j] * dx[j] / s;
            J[5][j] = gy[j] * dy[j] / s;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double mean = window_sum<SPL>(J[c]) / n;
#pragma unroll
            for (int j = 0; j < SPL; ++j) J[c][j] = active[j] ? J[c][j] - mean : 0.0;
        }
        double Hm[6][6], b[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
            for (int d = c; d < 6; ++d) {
                double p[SPL];
#pragma unroll
                for (int j = 0; j < SPL; ++j) p[j] = J[c][j] * J[d][j];
                Hm[c][d] = Hm[d][c] = window_sum<SPL>(p);
            }
            double p[SPL];
#pragma unroll
            for (int j = 0; j < SPL; ++j) p[j] = J[c][j] * res[j];
            b[c] = window_sum<SPL>(p);
        }
        double trace = Hm[0][0];
#pragma unroll
        for (int c = 1; c < 6; ++c) trace = trace + Hm[c][c];
        const double ridge = 1e-9 * trace;
#pragma unroll
        for (int c = 0; c < 6; ++c) Hm[c][c] = Hm[c][c] + ridge;
        double L[6][6], delta[6];
        if (!sfmlm::factor<6>(Hm, 0.0, L) || !sfmlm::solve<6>(L, b, delta))
            return write_result(a, o, lane, SFM_REFINE_SINGULAR, x0, y0, A0, NAN, solves);
        ++solves;
        t0 = t0 + delta[0];
        t1 = t1 + delta[1];
#pragma unroll
        for (int k = 0; k < 4; ++k) A[k] = A[k] + delta[2 + k];
        const double sx = t0 - x0, sy = t1 - y0;
        if (sx * sx + sy * sy > a.max_shift2) return write_result(a, o, lane, SFM_REFINE_DIVERGED, x0, y0, A0, NAN, solves);
        if (delta[0] * delta[0] + delta[1] * delta[1] < a.min_step2) break;
    }

    // the correlation at the final state
    if (!window_positions<SPL>(dx, dy, active, t0, t1, A, W, H, u, v))
        return write_result(a, o, lane, SFM_REFINE_OUTSIDE, x0, y0, A0, NAN, solves);
#pragma unroll
    for (int j = 0; j < SPL; ++j) I[j] = active[j] ? bilinear(image, W, H, u[j], v[j]) : 0.0;
    const double ss = centre<SPL>(I, active, n);
    if (ss == 0.0) return write_result(a, o, lane, SFM_REFINE_FLAT, x0, y0, A0, NAN, solves);
    const double s = sqrt(ss);
    double p[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) p[j] = T[j] * (I[j] / s);
    const double correlation = window_sum<SPL>(p);
    if (correlation >= a.min_correlation) return write_result(a, o, lane, SFM_REFINE_OK, t0, t1, A, correlation, solves);
    write_result(a, o, lane, SFM_REFINE_LOW_CORRELATION, x0, y0, A0, correlation, solves);
}

template <int SPL>
void launch(const RefineArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(refine_kernel<SPL>, dim3(sfmhost::grid_for(a.M, kObsPerBlock)), dim3(kBlock), 0, st, a);
}

}  // namespace

extern "C" {

int64_t sfm_refine_observations_workspace_bytes(int64_t planes) {
    if (planes < 0 || planes > sfmplanes::kMaxPlanes) return -1;
    sfmhost::Carver c{0, 0};
    c.take<DevPlane>(planes + 1);
    return c.at;
}

int sfm_refine_observations(const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, const uint8_t* pool, int64_t pool_bytes,
                            int64_t observations, const int32_t* plane, const int32_t* x, const int32_t* y, const int32_t* reference,
                            const double* warp0, int radius, int max_iterations, double min_step, double max_shift,
                            double min_correlation, double* xy, double* warp, double* correlation, int32_t* iterations,
                            int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (planes < 0 || images < 0 || pool_bytes < 0 || observations < 0 || workspace_bytes < 0)
        return fail(SFM_EINVAL, "sfm_refine_observations: negative size");
    if (planes > sfmplanes::kMaxPlanes) return fail(SFM_EINVAL, "sfm_refine_observations: more than 65535 planes");
    if (pool_bytes > 0x7FFFFFFFLL || images > 0x7FFFFFFFLL || observations > 0x7FFFFFFFLL)
        return fail(SFM_EINVAL, "sfm_refine_observations: the pool, the images and the observations must stay below 2^31");
    if (radius < kMinRadius || radius > kMaxRadius) return fail(SFM_EINVAL, "sfm_refine_observations: radius must be in 2..7");
    if (max_iterations < 1 || max_iterations > kMaxIterations)
        return fail(SFM_EINVAL, "sfm_refine_observations: max_iterations must be in 1..50");
    if (!(min_step > 0.0) || !isfinite(min_step)) return fail(SFM_EINVAL, "sfm_refine_observations: min_step must be positive and finite");
    if (!(max_shift > 0.0) || !isfinite(max_shift))
        return fail(SFM_EINVAL, "sfm_refine_observations: max_shift must be positive and finite");
    if (isnan(min_correlation)) return fail(SFM_EINVAL, "sfm_refine_observations: min_correlation is NaN");
    if (observations == 0) return SFM_OK;
    if (!plane_table || !pool || !plane || !x || !y || !reference || !warp0 || !xy || !warp || !correlation || !iterations || !status ||
        !workspace)
        return fail(SFM_EINVAL, "sfm_refine_observations: null pointer");
    if ((reinterpret_cast<uintptr_t>(plane) & 3u) != 0 || (reinterpret_cast<uintptr_t>(x) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(y) & 3u) != 0 || (reinterpret_cast<uintptr_t>(reference) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(iterations) & 3u) != 0 || (reinterpret_cast<uintptr_t>(status) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(warp0) & 7u) != 0 || (reinterpret_cast<uintptr_t>(xy) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(warp) & 7u) != 0 || (reinterpret_cast<uintptr_t>(correlation) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
        return fail(SFM_EINVAL, "sfm_refine_observations: workspace must be 16-byte, the double arrays 8-byte and the int32 arrays "
                                "4-byte aligned");
    if (workspace_bytes < sfm_refine_observations_workspace_bytes(planes))
        return fail(SFM_EINVAL, "sfm_refine_observations: workspace smaller than sfm_refine_observations_workspace_bytes(planes)");
    CheckedTable checked;
    if (sfmplanes::check_table("sfm_refine_observations", plane_table, planes, images, pool_bytes, checked) != SFM_OK) return SFM_EINVAL;
    SFM_REQUIRE_GRID("sfm_refine_observations", observations, kObsPerBlock, kBlock);

    hipStream_t st = (hipStream_t)stream;
    DevPlane* planes_dev = reinterpret_cast<DevPlane*>(workspace);
    // the table is pageable host memory: the copy has left it when the call returns
    if (hipMemcpyAsync(planes_dev, checked.table.data(), sizeof(DevPlane) * checked.table.size(), hipMemcpyHostToDevice, st) != hipSuccess)
        return check_launch("sfm_refine_observations: table upload");
    RefineArgs a;
    a.planes = planes_dev;
    a.pool = pool;
    a.plane = plane, a.x = x, a.y = y, a.reference = reference, a.warp0 = warp0;
    a.xy = xy, a.warp = warp, a.correlation = correlation, a.iterations = iterations, a.status = status;
    a.M = observations;
    a.n_planes = (int)planes;
    a.radius = radius;
    a.max_iterations = max_iterations;
    a.min_step2 = min_step * min_step;
    a.max_shift2 = max_shift * max_shift;
    a.min_correlation = min_correlation;
    const int count = (2 * radius + 1) * (2 * radius + 1);
    switch ((count + kWave - 1) / kWave) {
        case 1: launch<1>(a, st); break;
        case 2: launch<2>(a, st); break;
        case 3: launch<3>(a, st); break;
        default: launch<4>(a, st); break;
    }
    return check_launch("sfm_refine_observations");
}

}  // extern "C"
