// Descriptor matching of every image pair of a collection in one ragged call (definition:
// tests/graph_matching_oracle.py).  Integer kernels only (the ratio test is one double multiply and one compare), vector
// stores only, no atomics: partner and distance are bit-identical to the NumPy definition.
//
// The descriptors of all images lie image-major in one array (image i owns rows image_offset[i] .. image_offset[i + 1] - 1,
// the convention of sfm_track_build.hip); pair q = (i, j) matches the features of image i (its rows) against those of image j
// (its columns) and owns the output rows row_offset[q] .. row_offset[q + 1] - 1, one per feature of image i.
//
//   match_pairs_nearest_kernel   grid (row blocks of the largest image, pairs, 2 directions), 256 lanes, one row per lane;
//                                direction 1 swaps the two images.  The other image passes through the tile of
//                                sfm_hamming_tile.h 512 descriptors at a time, and the lane carries
//                                (best, arg, second) over ALL tiles itself: v < best moves best to second and takes the column,
//                                else v < second takes second.  Scanning in column order with strict comparisons leaves the
//                                smallest column of the smallest distance and the smallest distance among the other columns.
//                                No per-tile workspace, no combine launch.
//   match_pairs_decide_kernel    one thread per output row: its pair by binary search in row_offset, the distance bound, the
//                                ratio test against the row's runner-up and, with the cross-check, the column's nearest row
//                                and runner-up.  Thread t < pairs also writes pair_status[t].
//
//   match_pairs_guided_kernel   the guided sibling of the nearest kernel (definition:
//                                tests/guided_matching_oracle.py), same grid: the tile also carries the columns' K-normalised
//                                coordinates and a column enters a lane's summary only if the pair's verified model admits it:
//                                sfm::sed_value (kind 1) or sfmhg::transfer_error (kind 2) at most the pair's threshold, always
//                                evaluated with image i's feature first, in either direction.  The fp64 gate is lazy: a column
//                                with d >= second changes nothing whatever its admissibility, so only columns with d < second
//                                pay for it.  sfm_match_pairs_guided launches it in place of the nearest kernel.
//
// All kernels judge a pair with the same pair_view(): a pair that names an image out of range, twice the same image, an
// image whose offsets leave [0, features] or whose size exceeds max_image_features, or whose row_offset span is not its
// first image's size has status 1; no pointer is formed from it, no block works on it and its rows are -1.  The guided call
// adds kind_ok(): a model kind outside 0 .. 2 is refused in the same way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_hamming_tile.h"
#include "sfm_homography.h"
#include "sfm_math.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_for;

using sfmham::kCols;                                // descriptors of the other image per LDS tile
using sfmham::kRows;                                // rows per block, one per lane
constexpr int kNone = 0x7FFFFFFF;                   // no distance: above every Hamming distance (<= 256)
constexpr int64_t kMaxPairs = 65535;                // the grid's y extent

static_assert(sizeof(sfm_match_pairs_options) == 24, "sfm_match_pairs_options layout is part of the ABI");

struct In {
    int I, F, Q, rows, max_n;
    const int32_t* image_offset;   // [I + 1]
    const int32_t* pair_images;    // [Q, 2]
    const int64_t* row_offset;     // [Q + 1]
};

// direction 0: per output row; direction 1: per pair and column, pair q's column b at q * max_n + b
struct Ws {
    int32_t *best, *arg, *second, *col_arg, *col_second;
};

struct PairView {
    bool ok;
    int oi, ni, oj, nj;   // first descriptor and size of both images
    int64_t r0;           // first output row
};

// Everything pair q's indices are checked against before anything is read through them.
SFM_DEVICE PairView pair_view(const In& in, int q) {
    PairView v{false, 0, 0, 0, 0, 0};
    const int i = in.pair_images[2 * (int64_t)q], j = in.pair_images[2 * (int64_t)q + 1];
    if (i < 0 || i >= in.I || j < 0 || j >= in.I || i == j) return v;
    const int oi = in.image_offset[i], ei = in.image_offset[i + 1], oj = in.image_offset[j], ej = in.image_offset[j + 1];
    if (oi < 0 || ei < oi || ei > in.F || oj < 0 || ej < oj || ej > in.F) return v;
    if (ei - oi > in.max_n || ej - oj > in.max_n) return v;
    const int64_t r0 = in.row_offset[q], r1 = in.row_offset[q + 1];
    if (r0 < 0 || r1 > in.rows || r1 - r0 != ei - oi) return v;
    return PairView{true, oi, ei - oi, oj, ej - oj, r0};
}

__global__ __launch_bounds__(kRows) void match_pairs_nearest_kernel(In in, const uint4* __restrict__ desc,
                                                                    const uint8_t* __restrict__ ok, Ws ws) {
    __shared__ sfmham::Tile s_b;
    const int q = blockIdx.y, dir = blockIdx.z;
    const PairView p = pair_view(in, q);   // block-uniform
    if (!p.ok) return;
    const int self0 = dir ? p.oj : p.oi, n_self = dir ? p.nj : p.ni;
    const int other0 = dir ? p.oi : p.oj, n_other = dir ? p.ni : p.nj;
    const int row0 = blockIdx.x * kRows;
    if (row0 >= n_self) return;            // block-uniform and before the first barrier
    const int row = row0 + threadIdx.x;
    const sfmham::Row a = sfmham::load_row(desc, ok, self0 + min(row, n_self - 1));
    int best = kNone, arg = -1, second = kNone;
    for (int c0 = 0; c0 < n_other; c0 += kCols) {
        const int cols = min(kCols, n_other - c0);
        __syncthreads();                   // the previous tile has been scanned by every lane
        sfmham::stage(s_b, desc, ok, (int64_t)other0 + c0, cols);
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < cols; ++k) {
            const int d = SFM_HAMMING_DISTANCE(a, s_b, k);
            const int v = s_b.ok[k] ? d : kNone;       // an invalid column is below nothing
            if (v < best) {                          // strict: the first minimum keeps its column
                second = best;
                best = v;
                arg = c0 + k;
            } else if (v < second) {
                second = v;
            }
        }
    }
    if (row >= n_self) return;
    if (!a.valid) {
        best = second = kNone;
        arg = -1;
    }
    if (dir == 0) {
        const int64_t r = p.r0 + row;
        ws.best[r] = best;
        ws.arg[r] = arg;
        ws.second[r] = second;
    } else {
        const int64_t c = (int64_t)q * in.max_n + row;
        ws.col_arg[c] = arg;
        ws.col_second[c] = second;
    }
}

// What the guided call adds to a pair: per feature its K-normalised coordinates, per pair the verified model.
struct Guide {
    const double* xy;          // [F, 2]
    const double* model;       // [Q, 9] row-major
    const int32_t* kind;       // [Q]: 0 none, 1 essential, 2 homography (the view graph's codes)
    const double* threshold;   // [Q]
};
constexpr int kKindNone = 0, kKindEssential = 1, kKindHomography = 2;

// kind == nullptr: the unguided call, which has no kinds to refuse
SFM_DEVICE bool kind_ok(const int32_t* __restrict__ kind, int64_t q) { return kind == nullptr || (uint32_t)kind[q] <= 2u; }

// The pair's model in the form its error function takes; block-uniform, so it lives in scalar registers.
template <int KIND>
struct GuideModel {
    double m[9], g[9], thr;
    SFM_DEVICE GuideModel(const double* __restrict__ model, double threshold) : thr(threshold) {
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = model[i];
        if (KIND == kKindHomography) sfmhg::adjugate(m, g);
    }
    // one IEEE compare: false for a NaN error, model, coordinate or threshold
    SFM_DEVICE bool admits(double xa, double ya, double xb, double yb) const {
        const double e = KIND == kKindEssential ? sfm::sed_value(m, xa, ya, xb, yb) : sfmhg::transfer_error(m, g, xa, ya, xb, yb);
        return e <= thr;
    }
};

// The walk of match_pairs_nearest_kernel over the other image's tiles with the gate in front of the update.  `self` is the
// lane's own feature; dir 1 walks image i's features, so the tile's column is the error function's first point.
template <int KIND>
SFM_DEVICE void guided_walk(sfmham::TileXY& s_b, const GuideModel<KIND>& gm, const uint4* __restrict__ desc,
                            const uint8_t* __restrict__ ok, const double* __restrict__ xy, const sfmham::Row& a, double x, double y,
                            bool live, int dir, int other0, int n_other, int& best, int& arg, int& second) {
    for (int c0 = 0; c0 < n_other; c0 += kCols) {
        const int cols = min(kCols, n_other - c0);
        __syncthreads();                   // the previous tile has been scanned by every lane
        sfmham::stage(s_b, desc, ok, xy, (int64_t)other0 + c0, cols);
        __syncthreads();
#pragma unroll 2
        for (int k = 0; k < cols; ++k) {
            const int d = SFM_HAMMING_DISTANCE(a, s_b, k);
#ifdef SFM_GUIDED_GATE_EVERY_COLUMN   // experiment build: the gate in front of every column (the slower form)
            const double2 c = s_b.xy[k];
            const bool in = dir ? gm.admits(c.x, c.y, x, y) : gm.admits(x, y, c.x, c.y);
            const int v = s_b.ok[k] && in ? d : kNone;
            if (v < best) {
                second = best;
                best = v;
                arg = c0 + k;
            } else if (v < second) {
                second = v;
            }
            continue;
#endif
            // best <= second: a column with d >= second is below nothing, admitted or not
            if (live && s_b.ok[k] && d < second) {
                const double2 c = s_b.xy[k];
                if (dir ? gm.admits(c.x, c.y, x, y) : gm.admits(x, y, c.x, c.y)) {
                    if (d < best) {                  // strict: the first minimum keeps its column
                        second = best;
                        best = d;
                        arg = c0 + k;
                    } else {
                        second = d;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(kRows) void match_pairs_guided_kernel(In in, Guide guide, const uint4* __restrict__ desc,
                                                                   const uint8_t* __restrict__ ok, Ws ws) {
    __shared__ sfmham::TileXY s_b;
    const int q = blockIdx.y, dir = blockIdx.z;
    const PairView p = pair_view(in, q);   // block-uniform, like everything read through q
    if (!p.ok) return;
    const int kind = guide.kind[q];
    if ((uint32_t)kind > 2u) return;       // status 1: the decide kernel writes the rows
    if (kind == kKindNone && dir == 1) return;   // nothing is admitted: no row reaches its column's summary
    const int self0 = dir ? p.oj : p.oi, n_self = dir ? p.nj : p.ni;
    const int other0 = dir ? p.oi : p.oj, n_other = dir ? p.ni : p.nj;
    const int row0 = blockIdx.x * kRows;
    if (row0 >= n_self) return;            // block-uniform and before the first barrier
    const int row = row0 + threadIdx.x;
    const int64_t self = self0 + min(row, n_self - 1);
    const sfmham::Row a = sfmham::load_row(desc, ok, self);
    const double x = guide.xy[2 * self], y = guide.xy[2 * self + 1];
    const bool live = a.valid && row < n_self;
    int best = kNone, arg = -1, second = kNone;
    const double* model = guide.model + 9 * (int64_t)q;
    const double thr = guide.threshold[q];
    if (kind == kKindEssential)
        guided_walk(s_b, GuideModel<kKindEssential>(model, thr), desc, ok, guide.xy, a, x, y, live, dir, other0, n_other, best, arg,
                    second);
    else if (kind == kKindHomography)
        guided_walk(s_b, GuideModel<kKindHomography>(model, thr), desc, ok, guide.xy, a, x, y, live, dir, other0, n_other, best,
                    arg, second);
    if (row >= n_self) return;
#ifdef SFM_GUIDED_GATE_EVERY_COLUMN
    if (!a.valid) {
        best = second = kNone;
        arg = -1;
    }
#endif
    if (dir == 0) {
        const int64_t r = p.r0 + row;
        ws.best[r] = best;
        ws.arg[r] = arg;
        ws.second[r] = second;
    } else {
        const int64_t c = (int64_t)q * in.max_n + row;
        ws.col_arg[c] = arg;
        ws.col_second[c] = second;
    }
}

// d against the runner-up s: one IEEE multiply and one compare (the build keeps them apart: -ffp-contract=off)
SFM_DEVICE bool distinctive(int d, int s, bool use_ratio, double ratio) {
    if (!use_ratio || s == kNone) return true;
    return (double)d <= ratio * (double)s;
}

__global__ __launch_bounds__(kRows) void match_pairs_decide_kernel(In in, Ws ws, int max_distance, bool use_ratio, double ratio,
                                                                   bool cross_check, const int32_t* __restrict__ kind,
                                                                   int32_t* __restrict__ partner, int32_t* __restrict__ distance,
                                                                   int32_t* __restrict__ pair_status) {
    const int64_t t = (int64_t)blockIdx.x * kRows + threadIdx.x;
    if (t < in.Q) pair_status[t] = pair_view(in, (int)t).ok && kind_ok(kind, t) ? 0 : 1;
    if (t >= in.rows) return;
    int out_partner = -1, out_distance = -1;
    const int64_t q = pair_of_item(in.row_offset, in.Q, t);
    if (q >= 0) {
        const PairView p = pair_view(in, (int)q);
        const int64_t a = t - p.r0;
        if (p.ok && kind_ok(kind, q) && a >= 0 && a < p.ni) {
            const int best = ws.best[t], b = ws.arg[t];
            bool keep = best != kNone && best <= max_distance && distinctive(best, ws.second[t], use_ratio, ratio);
            if (keep && cross_check) {
                const int64_t c = q * in.max_n + b;   // 0 <= b < nj <= max_n: the nearest kernel wrote it
                keep = ws.col_arg[c] == (int)a && distinctive(best, ws.col_second[c], use_ratio, ratio);
            }
            if (keep) {
                out_partner = b;
                out_distance = best;
            }
        }
    }
    partner[t] = out_partner;
    distance[t] = out_distance;
}

struct Layout {
    Ws ws;
    int64_t total;
};

Layout layout(uintptr_t base, int64_t pairs, int64_t rows, int64_t max_n) {
    sfmhost::Carver c{base, 0};
    Layout L;
    L.ws.best = c.take<int32_t>(rows);
    L.ws.arg = c.take<int32_t>(rows);
    L.ws.second = c.take<int32_t>(rows);
    L.ws.col_arg = c.take<int32_t>(pairs * max_n);
    L.ws.col_second = c.take<int32_t>(pairs * max_n);
    L.total = c.at;
    return L;
}

bool sizes_ok(int64_t pairs, int64_t rows, int64_t max_n) {
    return pairs >= 0 && pairs <= kMaxPairs && rows >= 0 && rows <= 0x7FFFFFFFLL && max_n >= 0 && max_n <= 0x7FFFFFFFLL;
}

int refuse(const char* fn, const char* what) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", fn, what);
    return fail(SFM_EINVAL, msg);
}

// Both entry points: every check, then the two launches.  `guide` is null for sfm_match_pairs.
int match_pairs_call(const char* fn, const Guide* guide, int64_t images, int64_t features, int64_t pairs, int64_t rows,
                     int64_t max_image_features, const int32_t* image_offset, const uint8_t* desc, const uint8_t* ok,
                     const int32_t* pair_images, const int64_t* row_offset, const sfm_match_pairs_options* options,
                     int32_t* partner, int32_t* distance, int32_t* pair_status, void* workspace, int64_t workspace_bytes,
                     void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (images < 0 || features < 0 || pairs < 0 || rows < 0 || max_image_features < 0) return refuse(fn, "negative size");
    if (pairs > kMaxPairs) return refuse(fn, "at most 65535 pairs per call");
    if (images > 0x7FFFFFFE || features > 0x7FFFFFFF || rows > 0x7FFFFFFF || max_image_features > 0x7FFFFFFF)
        return refuse(fn, "images, features, rows and max_image_features must be below 2^31");
    if (rows > 0 && pairs == 0) return refuse(fn, "rows without pairs");
    if (!options) return refuse(fn, "null options");
    if (options->reserved != 0) return refuse(fn, "options.reserved must be 0");
    if (options->max_distance < 0 || options->max_distance > 256) return refuse(fn, "options.max_distance must be in 0..256");
    if ((options->use_ratio != 0 && options->use_ratio != 1) || (options->cross_check != 0 && options->cross_check != 1))
        return refuse(fn, "options.use_ratio and options.cross_check must be 0 or 1");
    if (options->use_ratio && !(options->ratio > 0.0 && options->ratio <= 1.7976931348623157e308))
        return refuse(fn, "options.ratio must be finite and positive");
    if (pairs == 0) return SFM_OK;   // no rows either: nothing to write
    if (!image_offset || !pair_images || !row_offset || !pair_status || !workspace || (features > 0 && (!desc || !ok)) ||
        (rows > 0 && (!partner || !distance)))
        return refuse(fn, "null pointer");
    if (guide && (!guide->model || !guide->kind || !guide->threshold || (features > 0 && !guide->xy)))
        return refuse(fn, "null pointer");
    if ((reinterpret_cast<uintptr_t>(desc) & 15u) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
        return refuse(fn, "desc and workspace must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(row_offset) & 7u) != 0 ||
        ((reinterpret_cast<uintptr_t>(image_offset) | reinterpret_cast<uintptr_t>(pair_images) |
          reinterpret_cast<uintptr_t>(partner) | reinterpret_cast<uintptr_t>(distance) |
          reinterpret_cast<uintptr_t>(pair_status)) & 3u) != 0)
        return refuse(fn, "row_offset must be 8-byte and the int32 arrays 4-byte aligned");
    if (guide && (((reinterpret_cast<uintptr_t>(guide->xy) | reinterpret_cast<uintptr_t>(guide->model) |
                    reinterpret_cast<uintptr_t>(guide->threshold)) & 7u) != 0 ||
                  (reinterpret_cast<uintptr_t>(guide->kind) & 3u) != 0))
        return refuse(fn, "xy, model and threshold must be 8-byte and model_kind 4-byte aligned");
    const Layout L = layout(reinterpret_cast<uintptr_t>(workspace), pairs, rows, max_image_features);
    if (workspace_bytes < L.total) return refuse(fn, "workspace smaller than sfm_match_pairs_workspace_bytes");
    const int64_t row_blocks = (max_image_features + kRows - 1) / kRows;
    if (!sfmhost::grid_fits(max_image_features, kRows, kRows, pairs, 2) ||
        !sfmhost::grid_fits(rows > pairs ? rows : pairs, kRows, kRows))
        return refuse(fn, "size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y/z)");

    const In in{(int)images, (int)features, (int)pairs, (int)rows, (int)max_image_features, image_offset, pair_images,
                row_offset};
    hipStream_t st = (hipStream_t)stream;
    const dim3 nearest_grid((unsigned)row_blocks, (unsigned)pairs, 2);
    if (row_blocks > 0 && guide)
        hipLaunchKernelGGL(match_pairs_guided_kernel, nearest_grid, dim3(kRows), 0, st, in, *guide,
                           reinterpret_cast<const uint4*>(desc), ok, L.ws);
    else if (row_blocks > 0)
        hipLaunchKernelGGL(match_pairs_nearest_kernel, nearest_grid, dim3(kRows), 0, st, in, reinterpret_cast<const uint4*>(desc),
                           ok, L.ws);
    hipLaunchKernelGGL(match_pairs_decide_kernel, dim3(grid_for(rows > pairs ? rows : pairs, kRows)), dim3(kRows), 0, st, in, L.ws,
                       (int)options->max_distance, options->use_ratio != 0, options->ratio, options->cross_check != 0,
                       guide ? guide->kind : nullptr, partner, distance, pair_status);
    return check_launch(fn);
}


}  // namespace

extern "C" {

int64_t sfm_match_pairs_workspace_bytes(int64_t pairs, int64_t rows, int64_t max_image_features) {
    if (!sizes_ok(pairs, rows, max_image_features)) return -1;
    return layout(0, pairs, rows, max_image_features).total;
}

int sfm_match_pairs(int64_t images, int64_t features, int64_t pairs, int64_t rows, int64_t max_image_features,
                    const int32_t* image_offset, const uint8_t* desc, const uint8_t* ok, const int32_t* pair_images,
                    const int64_t* row_offset, const sfm_match_pairs_options* options, int32_t* partner, int32_t* distance,
                    int32_t* pair_status, void* workspace, int64_t workspace_bytes, void* stream) {
    return match_pairs_call("sfm_match_pairs", nullptr, images, features, pairs, rows, max_image_features, image_offset, desc, ok,
                            pair_images, row_offset, options, partner, distance, pair_status, workspace, workspace_bytes, stream);
}

int sfm_match_pairs_guided(int64_t images, int64_t features, int64_t pairs, int64_t rows, int64_t max_image_features,
                           const int32_t* image_offset, const uint8_t* desc, const uint8_t* ok, const double* xy,
                           const int32_t* pair_images, const int64_t* row_offset, const double* model, const int32_t* model_kind,
                           const double* threshold, const sfm_match_pairs_options* options, int32_t* partner, int32_t* distance,
                           int32_t* pair_status, void* workspace, int64_t workspace_bytes, void* stream) {
    const Guide guide{xy, model, model_kind, threshold};
    return match_pairs_call("sfm_match_pairs_guided", &guide, images, features, pairs, rows, max_image_features, image_offset,
                            desc, ok, pair_images, row_offset, options, partner, distance, pair_status, workspace, workspace_bytes,
                            stream);
}

}  // extern "C"
