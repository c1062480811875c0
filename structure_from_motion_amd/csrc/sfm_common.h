// Shared host/device helpers of the libsfm_hip.so translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/sfm_hip.h"

namespace sfmhost {

// thread-local last-error text shared by all translation units (defined in sfm_kernels.hip)
char* error_buffer();
constexpr int kErrorBytes = 512;

inline int fail(int code, const char* msg) {
    snprintf(error_buffer(), kErrorBytes, "%s", msg);
    return code;
}

inline int check_launch(const char* what) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        snprintf(error_buffer(), kErrorBytes, "%s: %s", what, hipGetErrorString(err));
        return SFM_EHIP;
    }
    return SFM_OK;
}

// Limits of ONE launch (HIP on gfx950): at most 2^31-1 blocks and 2^32-1 threads along x, 65535 blocks along y/z.
// Kernels without a grid-stride loop need every work item covered by a block of their own: their entry points
// refuse sizes beyond that with SFM_EINVAL (SFM_REQUIRE_GRID) instead of silently covering a prefix.
// `per_block` work items per block of `threads` threads.
inline bool grid_fits(int64_t work, int64_t per_block, int64_t threads, int64_t y = 1, int64_t z = 1) {
    if (work < 0 || per_block <= 0 || threads <= 0) return false;
    if (work > (int64_t)1 << 60) return false;
    const int64_t g = (work + per_block - 1) / per_block;
    return g <= 0x7FFFFFFFLL && g * threads <= 0xFFFFFFFFLL && y <= 65535 && z <= 65535;
}

// blocks that cover `work` items exactly once (the caller has checked grid_fits)
inline unsigned grid_for(int64_t work, int64_t block) {
    const int64_t g = (work + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : g);
}

// capped grid for kernels that walk their items with a grid-stride loop
inline unsigned grid_stride(int64_t work, int64_t block, int64_t cap) {
    int64_t g = (work + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// `bytes` a power of two; a null pointer is aligned
inline bool aligned_to(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// A stack of `views` image planes of height x width that kernels index with int32 coordinates and an int32 pixel within a plane.
inline bool image_stack_ok(int64_t views, int64_t height, int64_t width) {
    return views >= 1 && views <= 0x7FFFFFFF && height >= 1 && width >= 1 && height <= 0x7FFFFFFF && width <= 0x7FFFFFFF &&
           height * width < ((int64_t)1 << 31);
}

// Bump allocation of a workspace in 256-byte aligned pieces from `base` (0: sizes only).
struct Carver {
    uintptr_t base;
    int64_t at;
    template <class T>
    T* take(int64_t count) {
        const int64_t o = at, bytes = count * (int64_t)sizeof(T);
        at = (o + (bytes > 0 ? bytes : 8) + 255) & ~(int64_t)255;
        return reinterpret_cast<T*>(base + o);
    }
};

}  // namespace sfmhost

#define SFM_REQUIRE_GRID(fn, work, per_block, ...)                                                     \
    do {                                                                                               \
        if (!sfmhost::grid_fits((work), (per_block), __VA_ARGS__))                                       \
            return sfmhost::fail(SFM_EINVAL, fn ": size exceeds what one launch covers (2^31-1 blocks, " \
                                                "2^32-1 threads in x; 65535 in y/z)");               \
    } while (0)

constexpr int kWave = 64;

// Sample index of a hypothesis, checked: an index outside [0, n) reads item 0 and flags the hypothesis.
__device__ __forceinline__ int64_t checked_index(int32_t i, int64_t n, bool& bad) {
    const bool out = i < 0 || (int64_t)i >= n;
    bad = bad || out;
    return out ? 0 : (int64_t)i;
}

// The pair that owns item i of a ragged layout (pair q owns items offset[q] .. offset[q + 1] - 1; the table holds pairs + 1
// non-decreasing entries), or -1 for an item no pair owns.
__device__ __forceinline__ int64_t pair_of_item(const int64_t* __restrict__ offset, int64_t pairs, int64_t i) {
    // the first k in [0, pairs] with offset[k] > i: item i belongs to pair k - 1 when 1 <= k <= pairs
    int64_t lo = 0, hi = pairs + 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (offset[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return (lo >= 1 && lo <= pairs) ? lo - 1 : -1;
}

// One correspondence in K-normalised coordinates: 32 bytes, read as two 16-byte loads.
struct alignas(32) Corr {
    double xa, ya, xb, yb;
};
