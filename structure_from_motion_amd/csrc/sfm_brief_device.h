// The oriented integer BRIEF descriptor of one feature, computed by one wave (definition:
// tests/brief_oracle.py): the body shared by brief_describe_kernel (csrc/sfm_brief.hip, one image, float64 features) and
// keypoint_describe_kernel (csrc/sfm_keypoints.hip, the pyramid plane of every keypoint candidate).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"

namespace sfmbrief {

constexpr int kPatchRadius = 15;                    // orientation disc and patch half-width
constexpr int kPatch = 2 * kPatchRadius + 1;        // 31
constexpr int kBoxSide = 5;                         // a sample is the sum of a 5 x 5 box
constexpr int kBox = kPatch - kBoxSide + 1;         // 27 box centres per axis: offsets -13 .. 13
constexpr int kReach = kBox / 2;                    // 13
constexpr int kTests = 256;
constexpr int kWords = kTests / 64;                 // descriptor: 4 x 64 bits = 32 bytes
static_assert(kTests == kWords * kWave, "one ballot per descriptor word");

// One wave (a block of kWave threads) describes feature (x, y) of `image` [height, width] into desc[0 .. kWords - 1], *ok and
// *angle_bin.  Every lane of the block calls it with the same arguments.
__device__ __forceinline__ void describe_feature(
    const uint8_t* __restrict__ image, int64_t height, int64_t width, double x, double y,
    const int32_t* __restrict__ offsets, const long long* __restrict__ boundaries, int bins,
    unsigned long long* __restrict__ desc, uint8_t* __restrict__ ok, uint8_t* __restrict__ angle_bin) {
    __shared__ uint8_t s_patch[kPatch * kPatch];
    __shared__ uint16_t s_rows[kPatch * kBox];      // horizontal 5-sums
    __shared__ uint16_t s_box[kBox * kBox];
    const int lane = threadIdx.x;
    const double xc = floor(x + 0.5), yc = floor(y + 0.5);
    // block-uniform.  NaN fails every comparison; the range test also bounds the int conversion below
    const bool valid = xc >= (double)kPatchRadius && xc <= (double)(width - kPatchRadius - 1) &&
                       yc >= (double)kPatchRadius && yc <= (double)(height - kPatchRadius - 1);
    if (!valid) {
        if (lane < kWords) desc[lane] = 0ull;
        if (lane == 0) {
            *ok = 0;
            *angle_bin = 0;
        }
        return;
    }
    const int64_t x0 = (int64_t)xc - kPatchRadius, y0 = (int64_t)yc - kPatchRadius;
    int m10 = 0, m01 = 0;                           // |m| <= 709 pixels * 15 * 255
    for (int idx = lane; idx < kPatch * kPatch; idx += kWave) {
        const int r = idx / kPatch, c = idx - r * kPatch;
        const int p = image[(y0 + r) * width + (x0 + c)];
        s_patch[idx] = (uint8_t)p;
        const int dx = c - kPatchRadius, dy = r - kPatchRadius;
        if (dx * dx + dy * dy <= kPatchRadius * kPatchRadius) {
            m10 += dx * p;
            m01 += dy * p;
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off, kWave);
        m01 += __shfl_xor(m01, off, kWave);
    }
    // bin b: cross(B[b-1], m) >= 0 and cross(B[b], m) < 0 — a 12 degree wedge, exactly one for m != 0, none for m = 0
    bool hit = false;
    if (lane < bins) {
        const int prev = lane == 0 ? bins - 1 : lane - 1;
        const long long px = boundaries[2 * prev], py = boundaries[2 * prev + 1];
        const long long qx = boundaries[2 * lane], qy = boundaries[2 * lane + 1];
        hit = (px * m01 - py * m10 >= 0) && (qx * m01 - qy * m10 < 0);
    }
    const unsigned long long hits = __ballot(hit);
    const int bin = hits ? __ffsll((long long)hits) - 1 : 0;
    __syncthreads();
    for (int idx = lane; idx < kPatch * kBox; idx += kWave) {
        const int r = idx / kBox, c = idx - r * kBox;
        int s = 0;
#pragma unroll
        for (int k = 0; k < kBoxSide; ++k) s += s_patch[r * kPatch + c + k];
        s_rows[idx] = (uint16_t)s;
    }
    __syncthreads();
    for (int idx = lane; idx < kBox * kBox; idx += kWave) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < kBoxSide; ++k) s += s_rows[idx + k * kBox];
        s_box[idx] = (uint16_t)s;
    }
    __syncthreads();
    auto coordinate = [](int32_t packed, int byte) {   // int8 of the packed (ax, ay, bx, by), held inside the box array
        const int v = (int)(int8_t)(packed >> (8 * byte));
        return min(max(v, -kReach), kReach) + kReach;
    };
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
        const int32_t o = offsets[(int64_t)bin * kTests + k * kWave + lane];
        const int a = s_box[coordinate(o, 1) * kBox + coordinate(o, 0)];
        const int b = s_box[coordinate(o, 3) * kBox + coordinate(o, 2)];
        const unsigned long long word = __ballot(a < b);
        if (lane == 0) desc[k] = word;
    }
    if (lane == 0) {
        *ok = 1;
        *angle_bin = (uint8_t)bin;
    }
}

}  // namespace sfmbrief
