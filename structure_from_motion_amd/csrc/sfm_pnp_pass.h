// What the dense PnP pass (sfm_pnp.hip) and the ragged registration of every view (sfm_register_views.hip)
// share: the data the pose fits read, the P3P solver, the scoring loop of one hypothesis per lane over a view's items, and the
// model of the winner's mask.  Moved here unchanged from sfm_pnp.hip, so that both calls run the same device routines in the
// same order and the ragged call's outputs are the single-view chain's bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"
#include "sfm_minimal_score.h"
#include "sfm_p3p.h"
#include "sfm_pnp.h"

namespace sfmpnp {

constexpr int kP3PSample = 4;   // P3P: three items solved for, the fourth picks the solution

// What the pose fits read besides the sample: the items of every batch entry and the camera.  The solvers are the
// `Solver` of sfmmin::minimal_fit_kernel (sfm_minimal_fit.h), named like the kernels they parameterise so that a profile
// filtered by "pnp" / "p3p" finds minimal_fit_kernel<pnp_dlt_solver, ...> and minimal_fit_kernel<p3p_solver, ...>.
struct PoseData {
    const double* pts;
    PnPCamera cam;
};

// P3P fit of one hypothesis (sfm_p3p.h) from sample indices idx[0..3]: SFM_FIT_DEGENERATE when items 0-2 are collinear or
// coincide or an index is out of range; otherwise the chosen model, or 12 NaNs when the sample has no solution (flag 0).
// One hypothesis per lane, all in registers: the up-to-four candidates are scored as they are made.
struct p3p_solver {
    static constexpr int kSample = kP3PSample, kModel = 12;
    static constexpr const char* kName = "minimal_fit_kernel<p3p_solver>";
    using Data = PoseData;
    SFM_DEVICE static Data from(const Data& data, int64_t first) { return Data{data.pts + first * kPnPFields, data.cam}; }
    SFM_DEVICE static int fit(const Data& data, int64_t b, int64_t n, const int32_t (&idx)[8], double (&out)[12]) {
        const double* __restrict__ pts = data.pts + b * n * kPnPFields;
        bool bad = false;
        const double* q0 = pts + checked_index(idx[0], n, bad) * kPnPFields;
        const double* q1 = pts + checked_index(idx[1], n, bad) * kPnPFields;
        const double* q2 = pts + checked_index(idx[2], n, bad) * kPnPFields;
        const double* q3 = pts + checked_index(idx[3], n, bad) * kPnPFields;
        const bool ok = sfmp3p::p3p_fit_one(q0, q1, q2, q3, data.cam, out);
        return (bad || !ok) ? SFM_FIT_DEGENERATE : 0;
    }
};

// A tile slot of the pose scorer: a point as three 16-byte words (512 x 48 B = 24 KiB).
struct alignas(16) TilePoint {
    double2 xy, zu, v_;
};

// The loop of sfmmin::score_hypothesis (sfm_minimal_score.h) written out for the pose — one hypothesis per lane (its model the
// 12 doubles at `model`, its sample the leading SAMPLE entries of `sample_row`), the n points at P staged through LDS in tiles
// read by broadcast, every point counted, the SAMPLE sample points then corrected.  All fp64 with the divisions of pnp_score: no
// fast path, so every value is the oracle's bit for bit and only the summation order differs.  Every lane of the block must
// call this with the same P and n (two barriers per tile).
template <int SAMPLE>
SFM_DEVICE sfmmin::HypothesisScore score_pose_hypothesis(TilePoint* tile, const double* __restrict__ P, int64_t n,
                                                         const double* __restrict__ model, const int32_t* __restrict__ sample_row,
                                                         const PnPCamera& cam, double thr) {
    using sfmmin::kScoreBlock;
    using sfmmin::kScoreTile;
    double m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = model[i];
    int c = 0;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t base = 0; base < n; base += kScoreTile) {
        const int count = (int)(n - base < kScoreTile ? n - base : kScoreTile);
        __syncthreads();  // the previous tile has been read by every lane
        for (int i = threadIdx.x; i < count; i += kScoreBlock) {
            const double* q = P + (base + i) * kPnPFields;
            tile[i].xy = make_double2(q[0], q[1]);
            tile[i].zu = make_double2(q[2], q[3]);
            tile[i].v_ = make_double2(q[4], 0.0);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < count; ++j) {
            const TilePoint t = tile[j];
            const double e = pnp_score(m, cam, t.xy.x, t.xy.y, t.zu.x, t.zu.y, t.v_.x);
            const bool in = e <= thr;
            c += in ? 1 : 0;
            a1 += in ? e : 0.0;
            a2 += in ? e * e : 0.0;
        }
    }
    bool bad = false;
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) {
        const double* q = P + checked_index(sample_row[k], n, bad) * kPnPFields;
        const double e = pnp_score(m, cam, q[0], q[1], q[2], q[3], q[4]);
        if (e <= thr) {
            --c;
        } else {
            a1 += e;
            a2 += e * e;
        }
    }
    return sfmmin::HypothesisScore{c, a1, a2};
}

// The `Model` of sfm_minimal_score.h for the winner's mask (sfmmin::mask_kernel): the pose and the camera in registers, a
// point as the five doubles the error reads.
struct pnp_model {
    using Stored = double;
    struct Item {
        double f[kPnPFields];
    };
    static constexpr int kStride = kPnPFields, kModel = 12;
    double m[12];
    PnPCamera cam;
    SFM_DEVICE pnp_model(const double* model, const PnPCamera& camera) : cam(camera) {
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = model[i];
    }
    SFM_DEVICE static void load(const double* items, int64_t i, Item& slot) {
#pragma unroll
        for (int k = 0; k < kPnPFields; ++k) slot.f[k] = items[i * kPnPFields + k];
    }
    SFM_DEVICE double error(const Item& t) const { return pnp_score(m, cam, t.f[0], t.f[1], t.f[2], t.f[3], t.f[4]); }
};

}  // namespace sfmpnp
