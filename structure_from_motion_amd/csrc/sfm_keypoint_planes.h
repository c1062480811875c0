// The plane table of the pixel pool: the record the kernels read and the one host check of the caller's
// table, shared by sfm_detect_keypoints, sfm_build_pyramid (sfm_keypoints.hip) and sfm_refine_observations
// (sfm_track_refine.hip).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "sfm_common.h"

namespace sfmplanes {

constexpr int kTileW = 64, kTileH = 16;             // pixels of a plane one block owns
constexpr int kMaxLevel = 11, kMinSide = 48, kMaxPlanes = 65535;

// the plane table as the kernels read it (built by the host from sfm_keypoint_plane)
struct DevPlane {
    int64_t offset;                                 // first pixel in the pool, and first entry in both score maps
    int32_t height, width;
    int32_t source;                                 // the plane of the same image one level down, -1 for level 0
    int32_t tiles_x;
    int32_t tile_start;                             // tiles of the planes before this one
    int32_t quota;
};

struct CheckedTable {
    std::vector<DevPlane> table;                    // planes + 1 records: the last one holds the total tile count
    std::vector<int64_t> level_first;               // first plane of every level, and the end
    int64_t tiles;
};

inline int fail_named(const char* fn, const char* msg) {
    snprintf(sfmhost::error_buffer(), sfmhost::kErrorBytes, "%s: %s", fn, msg);
    return SFM_EINVAL;
}

// The table: levels ascending, every plane above level 0 four fifths of its image's plane below, planes apart in the pool.
// SFM_OK and `out` filled, or SFM_EINVAL with the message under the caller's name `fn`.
inline int check_table(const char* fn, const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, int64_t pool_bytes,
                       CheckedTable& out) {
    std::vector<DevPlane>& table = out.table;
    table.assign((size_t)planes + 1, DevPlane{});
    std::vector<int32_t> below((size_t)images, -1), here((size_t)images, -1);   // per image: its plane one level down / at this level
    int64_t end = 0, tiles = 0;
    int level = 0;
    out.level_first.clear();
    out.level_first.push_back(0);
    for (int64_t p = 0; p < planes; ++p) {
        const sfm_keypoint_plane& in = plane_table[p];
        if (in.image < 0 || in.image >= images) return fail_named(fn, "a plane names no image");
        if (in.level < level || in.level > level + 1 || in.level > kMaxLevel)
            return fail_named(fn, "planes must come in ascending levels 0..11 without a gap");
        if (in.level > level) {
            level = in.level;
            below.swap(here);
            std::fill(here.begin(), here.end(), -1);
            out.level_first.push_back(p);
        }
        if (here[in.image] >= 0) return fail_named(fn, "an image has two planes of one level");
        if (in.height < 1 || in.width < 1) return fail_named(fn, "an empty plane");
        if (in.quota < 0 || in.reserved != 0) return fail_named(fn, "a negative quota or reserved != 0");
        int32_t source = -1;
        if (in.level > 0) {
            source = below[in.image];
            if (source < 0) return fail_named(fn, "a plane without the plane one level down");
            const DevPlane& s = table[(size_t)source];
            if (in.height != 4 * s.height / 5 || in.width != 4 * s.width / 5 || in.height < kMinSide || in.width < kMinSide)
                return fail_named(fn, "a level must be 4/5 of the one below and at least 48 x 48");
        }
        const int64_t size = (int64_t)in.height * in.width;
        if (in.offset < end || in.offset > pool_bytes || size > pool_bytes - in.offset)
            return fail_named(fn, "planes must lie in the pool in table order without overlap");
        end = in.offset + size;
        here[in.image] = (int32_t)p;
        DevPlane& o = table[(size_t)p];
        o.offset = in.offset;
        o.height = in.height;
        o.width = in.width;
        o.source = source;
        o.tiles_x = (in.width + kTileW - 1) / kTileW;
        o.tile_start = (int32_t)tiles;
        o.quota = in.quota;
        tiles += (int64_t)o.tiles_x * ((in.height + kTileH - 1) / kTileH);
        if (tiles > 0x7FFFFFFFLL) return fail_named(fn, "too many tiles for one launch");
    }
    out.level_first.push_back(planes);
    DevPlane& total = table[(size_t)planes];
    total = DevPlane{};
    total.tile_start = (int32_t)tiles;
    total.source = -1;
    out.tiles = tiles;
    return SFM_OK;
}

}  // namespace sfmplanes
