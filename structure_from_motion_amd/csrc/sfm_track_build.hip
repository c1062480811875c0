// Multi-view tracks from pairwise feature matches (the plain-Python oracle is tests/track_build_oracle.py).
// Integer kernels only.
//
// Features carry image-major global ids g = image_offset[i] + local.  The matches are the edges of a graph on the features;
// a component is named by its smallest id.  A component of one feature is UNMATCHED, one that holds two features of one
// image is a CONFLICT (dropped whole), every other component is a track.  Tracks are numbered in increasing component id
// and their observations listed by track, then by global id (hence by strictly increasing image inside a track).
//
// Launches, on one stream, no host synchronisation:
//   1. reset: the flag and the info record zeroed;
//   2. init, one thread per feature / offset: parent[g] = g, the image of g (binary search in image_offset), the conflict
//      marks zeroed, both offset arrays checked (monotone, first 0, last F resp. E);
//   3. union, one thread per match: its pair by binary search in match_offset, the images and local indices checked, then
//      a lock-free union-find (ECL-CC style).  Every access of `parent` in this launch is an agent-scope atomic: relaxed
//      loads, fetch_min for path halving, compare-and-swap to hook the larger root under the smaller.  parent[v] only ever
//      decreases, every value it ever held is in v's tree, and a failed CAS continues from the value it returned, so a
//      stale load costs a retry, never a wrong answer; each component's final root is its smallest id however the atomics
//      interleave.  Every loop is bounded (a round cap no correct run reaches and a wall-clock budget): running out sets
//      the flag to 2 and the info status to 2;
//   4. compress (new launch): key[g] = root of g, with the same atomic find;
//   5. group: a stable LSD radix sort of the feature ids by key (sfm_obs_order.h's ballot-ranked passes, 8 bits per pass);
//   6. runs: a position with the component and the image of its predecessor marks its component as a conflict;
//   7. flags: per sorted position, OK or not and the start of an OK run; the feature's status; the info counts;
//   8. two exclusive scans (sfm_obs_order.h): OK run starts -> track ids, OK positions -> observation slots;
//   9. write: the observation arrays (slots >= M to -1), track_of_feature, and the info totals; a set flag writes the
//      BAD_INDEX record instead.
// Every step before the last returns at once once the flag is set.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_obs_order.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;

constexpr int kThreads = 256;
constexpr int kCheckEvery = 256;   // find steps between two reads of the wall clock

static_assert(sizeof(sfm_build_tracks_info) == 48, "sfm_build_tracks_info layout is part of the ABI");

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct Layout {
    size_t flag, parent, img, key, mark, seq0, seq1, table, table_sum, ok_start, ok_pos, tile_sum, total;
};

Layout layout(int64_t F) {
    Layout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o = align256(o + bytes);
        return (size_t)at;
    };
    L.flag = take(4);
    L.parent = take(4 * F);
    L.img = take(4 * F);
    L.key = take(4 * F);
    L.mark = take(4 * F);
    L.seq0 = take(4 * F);
    L.seq1 = take(4 * F);
    L.table = take(4 * sfmorder::table_size(F));
    L.table_sum = take(4 * sfmorder::tiles(sfmorder::table_size(F)));
    L.ok_start = take(4 * (F + 1));
    L.ok_pos = take(4 * (F + 1));
    L.tile_sum = take(4 * sfmorder::tiles(F));
    L.total = (size_t)o;
    return L;
}

struct Ws {
    int32_t *flag, *parent, *img, *key, *mark, *ok_start, *ok_pos;
};

struct In {
    int I, F, Q, E;
    const int32_t* image_offset;   // [I + 1]
    const int32_t* pair_images;    // [Q, 2]
    const int32_t* match_offset;   // [Q + 1]
    const int32_t* match_index;    // [E, 2]
};

struct Out {
    int32_t* component;   // nullable
    int32_t* track;
    uint8_t* status;
    int32_t *camera_index, *point_index, *feature_index;
    sfm_build_tracks_info* info;
};

// the last i in [0, n] with off[i] <= v (off[0] <= v); in range whatever off holds
SFM_DEVICE int upper_index(const int32_t* __restrict__ off, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= v)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ void build_reset_kernel(int32_t* __restrict__ flag, sfm_build_tracks_info* __restrict__ info) {
    if (threadIdx.x == 0) {
        *flag = 0;
        *info = sfm_build_tracks_info{0, 0, 0, 0, 0, 0};
    }
}

// thread t: feature t, image offset t, match offset t
__global__ __launch_bounds__(kThreads) void build_init_kernel(In in, Ws ws) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t < in.F) {
        ws.parent[t] = t;
        // the image whose range holds t: the last i < I with off[i] <= t
        ws.img[t] = min(upper_index(in.image_offset, in.I - 1, t), in.I - 1);
        ws.mark[t] = 0;
    }
    bool bad = false;
    if (t <= in.I) {
        const int32_t v = in.image_offset[t];
        bad = bad || (t == 0 && v != 0) || (t == in.I && v != in.F) || (t < in.I && in.image_offset[t + 1] < v);
    }
    if (t <= in.Q) {
        const int32_t v = in.match_offset[t];
        bad = bad || (t == 0 && v != 0) || (t == in.Q && v != in.E) || (t < in.Q && in.match_offset[t + 1] < v);
    }
    if (bad) *ws.flag = 1;   // every offender stores the same value
}

SFM_DEVICE int32_t load_parent(int32_t* parent, int v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Bounds of one thread's loops: false once its wall-clock budget is spent
struct Budget {
    uint64_t start, ticks;
    int steps;
    SFM_DEVICE bool ok() {
        if (++steps % kCheckEvery != 0) return true;
        return (uint64_t)wall_clock64() - start <= ticks;
    }
};

// Root of v's tree.  Each step moves v's pointer to its grandparent (fetch_min: parent only decreases) and goes on from
// there, so v strictly decreases: at most F steps.  Loads may be stale; every value they return was once v's parent, so it
// is in v's tree.  Returns -1 when the budget runs out.
SFM_DEVICE int find_root(int32_t* parent, int v, Budget& b) {
    while (true) {
        const int p = load_parent(parent, v);
        if (p == v) return v;
        const int gp = load_parent(parent, p);
        if (gp == p) return p;
        __hip_atomic_fetch_min(parent + v, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = gp;
        if (!b.ok()) return -1;
    }
}

// Thread m: match m.  Its pair q is the last with match_offset[q] <= m (offsets checked by init: the flag is clear).
__global__ __launch_bounds__(kThreads) void build_union_kernel(In in, Ws ws, uint64_t budget_ticks) {
    if (*ws.flag) return;
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= in.E) return;
    const int q = upper_index(in.match_offset, in.Q - 1, m);
    const int ia = in.pair_images[2 * (int64_t)q], ib = in.pair_images[2 * (int64_t)q + 1];
    if (ia < 0 || ia >= in.I || ib < 0 || ib >= in.I || ia == ib) {
        *ws.flag = 1;
        return;
    }
    const int la = in.match_index[2 * (int64_t)m], lb = in.match_index[2 * (int64_t)m + 1];
    const int oa = in.image_offset[ia], ob = in.image_offset[ib];
    if (la < 0 || la >= in.image_offset[ia + 1] - oa || lb < 0 || lb >= in.image_offset[ib + 1] - ob) {
        *ws.flag = 1;
        return;
    }
    Budget b{(uint64_t)wall_clock64(), budget_ticks, 0};
    int ra = find_root(ws.parent, oa + la, b), rb = find_root(ws.parent, ob + lb, b);
    // Each failed round means max(ra, rb) was hooked meanwhile and the next round's max is below it: at most F rounds.
    for (int round = 0; ra >= 0 && rb >= 0 && ra != rb; ++round) {
        const int hi = max(ra, rb), lo = min(ra, rb);
        if (round > in.F || (uint64_t)wall_clock64() - b.start > b.ticks) {
            ra = -1;
            break;
        }
        int32_t expected = hi;
        if (__hip_atomic_compare_exchange_strong(ws.parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        // hi is no root: go on from the parent the CAS returned (authoritative), not from a new load
        ra = find_root(ws.parent, expected, b);
        rb = find_root(ws.parent, lo, b);
    }
    if (ra < 0 || rb < 0) *ws.flag = 2;   // bounded loop gave up: every offender stores the same value
}

// key[g] = root of g (the smallest id of its component); the identity sequence the radix passes sort
__global__ __launch_bounds__(kThreads) void build_compress_kernel(int F, Ws ws, int32_t* __restrict__ component,
                                                                  int32_t* __restrict__ seq0, uint64_t budget_ticks) {
    if (*ws.flag) return;
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= F) return;
    Budget b{(uint64_t)wall_clock64(), budget_ticks, 0};
    const int r = find_root(ws.parent, g, b);
    if (r < 0) {
        *ws.flag = 2;
        return;
    }
    ws.key[g] = r;
    if (component) component[g] = r;
    seq0[g] = g;
}

// Sorted position i (s = the sorted feature ids): the same component and image as position i - 1 is a conflict
__global__ __launch_bounds__(kThreads) void build_runs_kernel(int F, const int32_t* __restrict__ s, Ws ws) {
    if (*ws.flag) return;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= F || i == 0) return;
    const int g = s[i], h = s[i - 1];
    const int c = ws.key[g];
    if (ws.key[h] == c && ws.img[h] == ws.img[g]) ws.mark[c] = 1;   // every offender stores the same value
}

// Sorted position i: status of its feature, OK run start and OK position (0 / 1, scanned next), the info counts
__global__ __launch_bounds__(kThreads) void build_flags_kernel(int F, const int32_t* __restrict__ s, Ws ws, Out out) {
    __shared__ unsigned long long sums[3];
    if (*ws.flag) return;
    if (threadIdx.x < 3) sums[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * kThreads + threadIdx.x;
    bool start = false, single = false, conflict = false;
    if (i < F) {
        const int g = s[i], c = ws.key[g];
        start = i == 0 || ws.key[s[i - 1]] != c;
        const bool end = i == F - 1 || ws.key[s[i + 1]] != c;
        single = start && end;
        conflict = ws.mark[c] != 0;
        const bool ok = !single && !conflict;
        ws.ok_start[i] = ok && start;
        ws.ok_pos[i] = ok;
        out.status[g] = (uint8_t)(single ? SFM_BUILD_UNMATCHED : conflict ? SFM_BUILD_CONFLICT : SFM_BUILD_OK);
        if (!ok) out.track[g] = -1;
    }
    // components of two or more features, conflict components, unmatched features: a ballot per wave, a sum per block
    const uint64_t multi = __ballot(start && !single), bad = __ballot(start && conflict), alone = __ballot(single);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (multi) atomicAdd(&sums[0], (unsigned long long)__popcll(multi));
        if (bad) atomicAdd(&sums[1], (unsigned long long)__popcll(bad));
        if (alone) atomicAdd(&sums[2], (unsigned long long)__popcll(alone));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sums[0]) atomicAdd(reinterpret_cast<unsigned long long*>(&out.info->components), sums[0]);
        if (sums[1]) atomicAdd(reinterpret_cast<unsigned long long*>(&out.info->conflicts), sums[1]);
        if (sums[2]) atomicAdd(reinterpret_cast<unsigned long long*>(&out.info->unmatched), sums[2]);
    }
}

// Sorted position i (after the scans: ok_start and ok_pos hold exclusive offsets, [F] their totals); thread 0 the totals.
// A set flag: every feature BAD_INDEX (1; or the gave-up record, 2), no observations.
__global__ __launch_bounds__(kThreads) void build_write_kernel(int F, const int32_t* __restrict__ s, Ws ws, Out out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int flag = *ws.flag;
    if (flag) {
        if (i < F) {
            out.status[i] = (uint8_t)SFM_BUILD_BAD_INDEX;
            out.track[i] = -1;
            if (out.component) out.component[i] = -1;
            out.camera_index[i] = out.point_index[i] = out.feature_index[i] = -1;
        }
        if (i == 0) *out.info = sfm_build_tracks_info{flag, 0, 0, 0, 0, 0};
        return;
    }
    const int32_t tracks = F > 0 ? ws.ok_start[F] : 0, M = F > 0 ? ws.ok_pos[F] : 0;
    if (i == 0) {
        out.info->tracks = tracks;
        out.info->observations = M;
    }
    if (i >= F) return;
    if (i >= M) out.camera_index[i] = out.point_index[i] = out.feature_index[i] = -1;
    const int32_t slot = ws.ok_pos[i];
    if (ws.ok_pos[i + 1] == slot) return;   // not OK
    const int g = s[i];
    const int32_t t = ws.ok_start[i + 1] - 1;   // OK run starts up to and including i, less one
    out.camera_index[slot] = ws.img[g];
    out.point_index[slot] = t;
    out.feature_index[slot] = g;
    out.track[g] = t;
}

}  // namespace

extern "C" {

int64_t sfm_build_tracks_workspace_bytes(int64_t images, int64_t features, int64_t matches) {
    if (images < 0 || features < 0 || matches < 0 || images > 0x7FFFFFFE || features > 0x7FFFFFFE || matches > 0x7FFFFFFF)
        return -1;
    return (int64_t)layout(features).total;
}

int sfm_build_tracks(int64_t images, int64_t features, int64_t pairs, int64_t matches, const int32_t* image_offset,
                     const int32_t* pair_images, const int32_t* match_offset, const int32_t* match_index, int32_t* component,
                     int32_t* track, uint8_t* status, int32_t* camera_index, int32_t* point_index, int32_t* feature_index,
                     sfm_build_tracks_info* info, void* workspace, int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (images < 0 || features < 0 || pairs < 0 || matches < 0) return fail(SFM_EINVAL, "sfm_build_tracks: negative size");
    if (images > 0x7FFFFFFE || features > 0x7FFFFFFE || pairs > 0x7FFFFFFE || matches > 0x7FFFFFFF)
        return fail(SFM_EINVAL, "sfm_build_tracks: images, features and pairs must be below 2^31 - 1, matches below 2^31");
    if (matches > 0 && pairs == 0) return fail(SFM_EINVAL, "sfm_build_tracks: matches without pairs");
    if (!info || !workspace || !image_offset || !match_offset || (pairs > 0 && !pair_images) ||
        (matches > 0 && !match_index) ||
        (features > 0 && (!track || !status || !camera_index || !point_index || !feature_index)))
        return fail(SFM_EINVAL, "sfm_build_tracks: null pointer");
    const int64_t I = images, F = features, Q = pairs, E = matches;
    const Layout L = layout(F);
    if (workspace_bytes < (int64_t)L.total) return fail(SFM_EINVAL, "sfm_build_tracks: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_build_tracks: workspace must be 16-byte aligned");
    // one second of wall clock per thread (the counter's rate from the device; 100 MHz where the query fails)
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
        khz <= 0)
        khz = 100000;
    (void)hipGetLastError();
    const uint64_t budget = (uint64_t)khz * 1000u;

    hipStream_t st = (hipStream_t)stream;
    char* b = static_cast<char*>(workspace);
    auto at = [&](size_t off) { return reinterpret_cast<int32_t*>(b + off); };
    const Ws ws{at(L.flag), at(L.parent), at(L.img), at(L.key), at(L.mark), at(L.ok_start), at(L.ok_pos)};
    const In in{(int)I, (int)F, (int)Q, (int)E, image_offset, pair_images, match_offset, match_index};
    const Out out{component, track, status, camera_index, point_index, feature_index, info};
    // the radix passes of sfm_obs_order.h: keys = component ids, the flag stops them
    const sfmorder::PointOrder o{nullptr, nullptr, nullptr, nullptr, ws.flag};
    const sfmorder::CameraOrder co{ws.key, at(L.seq0), at(L.seq1), at(L.table), at(L.table_sum), nullptr, nullptr, nullptr};

    hipLaunchKernelGGL(build_reset_kernel, dim3(1), dim3(kWave), 0, st, ws.flag, info);
    hipLaunchKernelGGL(build_init_kernel, dim3(sfmhost::grid_for(std::max(F, std::max(I, Q) + 1), kThreads)), dim3(kThreads), 0,
                       st, in, ws);
    if (E > 0)
        hipLaunchKernelGGL(build_union_kernel, dim3(sfmhost::grid_for(E, kThreads)), dim3(kThreads), 0, st, in, ws, budget);
    const int32_t* s = co.seq0;
    if (F > 0) {
        const unsigned fgrid = sfmhost::grid_for(F, kThreads);
        hipLaunchKernelGGL(build_compress_kernel, dim3(fgrid), dim3(kThreads), 0, st, (int)F, ws, component, co.seq0, budget);
        const int rtiles = (int)sfmorder::radix_tiles(F);
        int32_t *src = co.seq0, *dst = co.seq1;
        for (int shift = 0; ((F - 1) >> shift) > 0; shift += sfmorder::kRadixBits) {
            hipLaunchKernelGGL(sfmorder::order_radix_kernel<false>, dim3(rtiles), dim3(sfmorder::kRadixTile), 0, st, (int)F, shift,
                               rtiles, src, dst, o, co);
            sfmorder::launch_scan(co.table, sfmorder::table_size(F) - 1, co.table_sum, ws.flag, st);
            hipLaunchKernelGGL(sfmorder::order_radix_kernel<true>, dim3(rtiles), dim3(sfmorder::kRadixTile), 0, st, (int)F, shift,
                               rtiles, src, dst, o, co);
            std::swap(src, dst);
        }
        s = src;
        int32_t* tile_sum = at(L.tile_sum);
        hipLaunchKernelGGL(build_runs_kernel, dim3(fgrid), dim3(kThreads), 0, st, (int)F, s, ws);
        hipLaunchKernelGGL(build_flags_kernel, dim3(fgrid), dim3(kThreads), 0, st, (int)F, s, ws, out);
        sfmorder::launch_scan(ws.ok_start, F, tile_sum, ws.flag, st);
        sfmorder::launch_scan(ws.ok_pos, F, tile_sum, ws.flag, st);
    }
    hipLaunchKernelGGL(build_write_kernel, dim3(sfmhost::grid_for(F, kThreads)), dim3(kThreads), 0, st, (int)F, s, ws, out);
    return check_launch("sfm_build_tracks");
}

}  // extern "C"
