// Model selection (reference lib/ransac/ransac.py:75-86) and the winner's inlier mask (:70-76) as device routines of the
// selection kernels (sfm_kernels.hip): the candidate and its ordering rule, the wave- and block-level folds, the finished record,
// the mask value of a point, and the hand-off by which the selecting blocks of ONE launch fold their candidates and release the
// blocks that write the mask.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_math.h"

namespace sfmsel {

// "no model" key: above every finite non-negative double's bit pattern, and still positive when the
// record is viewed as int64 (so a cross-GPU MIN on int64 works).
constexpr uint64_t kNoModelKey = 0x7FFFFFFFFFFFFFFFull;

// Key of a hypothesis from its count and sums: the bits of its aggregated error, or kNoModelKey where it does not compete.
SFM_DEVICE uint64_t key_of(int ch, double sum1, double sum2, bool flagged, double min_extra, int aggregation, int sample_size = 8) {
    const double err = sfmfit::aggregate_error(aggregation, ch, sum1, sum2, sample_size);
    // ransac.py:75 gate and :83 strict compare against an initial +inf: NaN and inf never win.
    // Hypotheses whose sample was flagged degenerate never compete (the reference aborts on them).
    const bool ok = ((double)ch >= min_extra) && (err < INFINITY) && !flagged;
    uint64_t bits = (uint64_t)__double_as_longlong(err);
    if (bits == 0x8000000000000000ull) bits = 0;  // -0.0 orders as +0.0
    return ok ? bits : kNoModelKey;
}
SFM_DEVICE bool is_flagged(const int32_t* flags, int64_t h) { return flags != nullptr && flags[h] != 0; }
SFM_DEVICE uint64_t hypothesis_key(const int32_t* cnt, const double* s1, const double* s2, const int32_t* flags,
                                   int64_t h, double min_extra, int aggregation, bool& flagged, int sample_size = 8) {
    flagged = is_flagged(flags, h);
    return key_of(cnt[h], s1[h], s2[h], flagged, min_extra, aggregation, sample_size);
}

// What a selection carries from one hypothesis to all of them: the best key and its index, and the flag statistics.  32 bytes:
// also the partial record a selecting block leaves for the hand-off below.
struct Candidate {
    uint64_t key;
    int64_t best, first_flagged;
    int32_t n_flagged, pad;

    static SFM_DEVICE Candidate none() { return Candidate{kNoModelKey, INT64_MAX, INT64_MAX, 0, 0}; }   // merge's neutral element
    // one hypothesis (a non-competing one carries no index: best == INT64_MAX exactly where key == kNoModelKey)
    static SFM_DEVICE Candidate of(uint64_t key, int64_t h, bool flagged) {
        return Candidate{key, key != kNoModelKey ? h : INT64_MAX, flagged ? h : INT64_MAX, flagged ? 1 : 0, 0};
    }
    // The rule of ransac.py:83-86: lowest key, then lowest index; first flagged index and flag count of both.
    SFM_DEVICE void merge(const Candidate& o) {
        if (o.key < key || (o.key == key && o.best < best)) {
            key = o.key;
            best = o.best;
        }
        first_flagged = o.first_flagged < first_flagged ? o.first_flagged : first_flagged;
        n_flagged += o.n_flagged;
    }
    SFM_DEVICE bool found() const { return key != kNoModelKey && best != INT64_MAX; }
};
static_assert(sizeof(Candidate) == 32, "a partial record of the hand-off is 32 bytes");

// The finished record of a candidate over hypotheses [h_offset, ...): global indices, the "none" sentinels.  best_cnt: the
// winner's count (read only where c.found()).
SFM_DEVICE sfm_select_result finish_record(const Candidate& c, int64_t h_offset, int32_t best_cnt) {
    const bool found = c.found();
    sfm_select_result r;
    r.key = found ? c.key : kNoModelKey;
    r.best_h = found ? c.best + h_offset : -1;
    r.best_err = found ? __longlong_as_double((long long)c.key) : INFINITY;
    r.first_flagged = c.first_flagged != INT64_MAX ? c.first_flagged + h_offset : INT64_MAX;
    r.n_flagged = c.n_flagged;
    r.best_cnt = found ? best_cnt : 0;
    return r;
}

// One thread's candidate over hypotheses first, first + stride, ...: IN_FLIGHT of them per trip with their loads issued
// together (the loop is pure load latency otherwise).  key(h, flagged) -> the key of hypothesis h.  (h increases, so among
// equal keys merge keeps the earliest.)
template <int IN_FLIGHT, class Key>
SFM_DEVICE Candidate scan_candidates(int64_t first, int64_t stride, int64_t h_count, Key key) {
    Candidate c = Candidate::none();
    for (int64_t h0 = first; h0 < h_count; h0 += IN_FLIGHT * stride) {
        uint64_t k[IN_FLIGHT];
        bool flagged[IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < IN_FLIGHT; ++u) {
            const int64_t h = h0 + u * stride;
            flagged[u] = false;
            k[u] = h < h_count ? key(h, flagged[u]) : kNoModelKey;
        }
#pragma unroll
        for (int u = 0; u < IN_FLIGHT; ++u) c.merge(Candidate::of(k[u], h0 + u * stride, flagged[u]));
    }
    return c;
}

// Wave-level fold of candidates: four DPP row rotations leave every lane of a 16-lane row with the row's result, the four rows
// are then read out with v_readlane and folded in row order.  All VALU: the __shfl_xor butterfly this replaces went
// through the LDS crossbar (ds_bpermute) six times in a dependent chain with seven words each — most of what a
// latency-bound selection block waited on.
template <int N>
SFM_DEVICE uint64_t dpp_ror_u64(uint64_t x) {
    const uint32_t lo = (uint32_t)sfm::dpp_row_ror<N>((int)(uint32_t)x), hi = (uint32_t)sfm::dpp_row_ror<N>((int)(uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}
SFM_DEVICE uint64_t read_lane_u64(uint64_t x, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}
template <int N>
SFM_DEVICE Candidate dpp_ror(const Candidate& c) {
    Candidate o = c;
    o.key = dpp_ror_u64<N>(c.key);
    o.best = (int64_t)dpp_ror_u64<N>((uint64_t)c.best);
    o.first_flagged = (int64_t)dpp_ror_u64<N>((uint64_t)c.first_flagged);
    o.n_flagged = sfm::dpp_row_ror<N>(c.n_flagged);
    return o;
}
SFM_DEVICE Candidate read_lane(const Candidate& c, int lane) {
    Candidate o = c;
    o.key = read_lane_u64(c.key, lane);
    o.best = (int64_t)read_lane_u64((uint64_t)c.best, lane);
    o.first_flagged = (int64_t)read_lane_u64((uint64_t)c.first_flagged, lane);
    o.n_flagged = __builtin_amdgcn_readlane(c.n_flagged, lane);
    return o;
}
SFM_DEVICE void wave_fold(Candidate& c) {
    c.merge(dpp_ror<8>(c));
    c.merge(dpp_ror<4>(c));
    c.merge(dpp_ror<2>(c));
    c.merge(dpp_ror<1>(c));
    // rows 1..3 into row 0's result (every lane ends up with the wave's result)
    Candidate r = read_lane(c, 0);
#pragma unroll
    for (int row = 1; row < 4; ++row) r.merge(read_lane(c, 16 * row));
    c = r;
}

// Shared-memory scratch of block_combine for a block of THREADS threads.
template <int THREADS>
struct SelectScratch {
    Candidate wave[THREADS / kWave];
};

// Block-wide fold of per-thread candidates; on return thread 0 holds the block's result.  SCRATCH_FREE: this is the block's
// first fold through `sh` (block_select: a 1024-thread block's smallest passes are a chain of ~4 us kernels, and a barrier
// nobody needs is not free there); otherwise a barrier comes first.
template <int THREADS, bool SCRATCH_FREE = false>
__device__ __forceinline__ void block_combine(Candidate& c, SelectScratch<THREADS>& sh) {
    wave_fold(c);
    if (!SCRATCH_FREE) __syncthreads();  // the scratch may still be read from a previous fold
    if ((threadIdx.x & (kWave - 1)) == 0) sh.wave[threadIdx.x / kWave] = c;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < THREADS / kWave; ++w) c.merge(sh.wave[w]);
}

// The whole selection over h_count hypotheses by ONE block of THREADS threads: lexicographic minimum of (error bits,
// index) — lowest aggregated error among gated hypotheses, earliest index on ties — plus the flag statistics.
// Thread 0 writes the record.  Returns (to every thread) the winner's LOCAL index, or -1.
template <int THREADS>
__device__ __forceinline__ int64_t block_select(const int32_t* __restrict__ cnt, const double* __restrict__ s1,
                                                const double* __restrict__ s2, const int32_t* __restrict__ flags,
                                                int64_t h_count, int64_t h_offset, double min_extra, int aggregation,
                                                sfm_select_result* __restrict__ record, SelectScratch<THREADS>& sh,
                                                int64_t* sh_winner, int sample_size = 8) {
    Candidate c = scan_candidates<4>(threadIdx.x, THREADS, h_count, [&](int64_t h, bool& flagged) {
        return hypothesis_key(cnt, s1, s2, flags, h, min_extra, aggregation, flagged, sample_size);
    });
    block_combine<THREADS, /*SCRATCH_FREE=*/true>(c, sh);
    if (threadIdx.x == 0) {
        *record = finish_record(c, h_offset, c.found() ? cnt[c.best] : 0);
        *sh_winner = c.found() ? c.best : -1;
    }
    __syncthreads();
    return *sh_winner;
}

// Mask value of point i (p) under the model e whose sample is the SAMPLE items at smp: 2 for a sample point, 1 for another point
// with sed <= thr, 0 otherwise.
template <int SAMPLE>
SFM_DEVICE uint8_t mask_value(const double* e, const int32_t* smp, const Corr& p, int64_t i, double thr) {
    const double sed = sfm::sed_value(e, p.xa, p.ya, p.xb, p.yb);
    bool in_sample = false;
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) in_sample |= (smp[k] == (int32_t)i);
    return in_sample ? 2 : ((sed <= thr) ? 1 : 0);
}

// mask[i] = mask_value of hypothesis h (its sample: the first SAMPLE entries of its row of S: 8 for the eight-point fit, 6 for
// the five-point fit); all zero for h outside [0, h_count).
// Points i = first, first + stride, ... (a block- or grid-stride walk).
template <int UNROLL = 1, int SAMPLE = 8>
__device__ __forceinline__ void write_inlier_mask(const Corr* __restrict__ pts, int64_t n, const double* __restrict__ E,
                                                  const int32_t* __restrict__ S, int64_t h_count, int64_t h, double thr,
                                                  uint8_t* __restrict__ out, int64_t first, int64_t stride) {
    if (h < 0 || h >= h_count) {
        for (int64_t i = first; i < n; i += stride) out[i] = 0;
        return;
    }
    double e[9];
    int32_t smp[SAMPLE];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = E[h * 9 + k];
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) smp[k] = S[h * 8 + k];
    // UNROLL points per trip with their loads issued together (a single block walking many points is load-latency bound)
    for (int64_t i0 = first; i0 < n; i0 += stride * UNROLL) {
        Corr p[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int64_t i = i0 + u * stride;
            p[u] = pts[i < n ? i : n - 1];
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n) out[i] = mask_value<SAMPLE>(e, smp, p[u], i, thr);
        }
    }
}

// Hand-off between the blocks of ONE launch (select_grid_kernel, sfm_kernels.hip): every selecting block leaves its candidate as
// a partial record and arrives on an agent-scope counter (cdna_hip_programming.md Guideline 16, counter form; 32 arrivals in
// a small pass and at most 256 in a large one, so a single counter does not serialise anything); the block that
// arrives last folds the partial records, publishes the finished record and raises a flag; the blocks that write the winner's
// mask — behind the selecting ones in the same launch — wait for that flag.  The state is caller-provided memory whose first
// 64-byte line is zero when the launch begins:
//   word 0 of the line: arrival counter;  word 8: "record published" flag;  byte 64 on: one 32-byte partial record per block
// Protocol: partial records and the record are written with relaxed agent-scope atomic stores (write-through); the arrival is
// a RELEASE (this block's stores — its partial record, and anything else it wrote for the last arriver — are visible before the
// count); the last arriver alone takes ONE acquire fence — not one per arrival —; the flag is a release store behind the record;
// a waiting block polls the flag RELAXED (each poll a load that bypasses the caches, nothing else) with s_sleep between polls and
// takes ONE acquire fence once it is up: with ~200 blocks polling, an acquire per poll invalidates the XCD's L2 under the
// selecting blocks' loads (profiles/r05).
// Residency: the wait assumes that every selecting block gets to run while mask blocks of the same launch occupy the chip.  A
// small pass launches at most 64 blocks, resident together on any MI355X; a large pass's blocks are all resident together up to
// n ~ 524 288 points, and beyond that the wait rests on the selecting blocks (the lowest block indices) being dispatched first.  Should the flag
// not arrive within kMaxFlagPolls polls the waiting block gives up (await -> false) and its caller fills its slice of the mask
// with 0xFF, a value no mask holds, rather than hanging the GPU.
struct Handoff {
    static constexpr int kFlagWord = 8;        // unsigned index: the flag shares the counter's 64-byte line
    static constexpr int kPartialOffset = 64;  // bytes: partial records behind that line
    static constexpr int kMaxFlagPolls = 1 << 22;

    unsigned* counter;
    unsigned* flag;
    Candidate* partial;

    SFM_DEVICE explicit Handoff(unsigned char* state)
        : counter(reinterpret_cast<unsigned*>(state)), flag(counter + kFlagWord),
          partial(reinterpret_cast<Candidate*>(state + kPartialOffset)) {}
    static constexpr int64_t state_bytes(int blocks) { return kPartialOffset + blocks * (int64_t)sizeof(Candidate); }

    // ONE thread of selecting block `block` of `blocks`: leaves the block's candidate and arrives.  True: this block is the last.
    SFM_DEVICE bool arrive(const Candidate& c, int block, int blocks) const {
        Candidate* out = partial + block;
        __hip_atomic_store(&out->key, c.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&out->best, c.best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&out->first_flagged, c.first_flagged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&out->n_flagged, c.n_flagged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned arrived = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = arrived == (unsigned)blocks - 1;
        if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        return last;
    }
    // Every thread of the last arriver (behind a barrier that follows arrive): thread t's share of the `blocks` partial records.
    SFM_DEVICE Candidate gather(int blocks) const {
        return (int)threadIdx.x < blocks ? partial[threadIdx.x] : Candidate::none();
    }
    // ONE thread of the last arriver: the record, then the flag that publishes it.
    SFM_DEVICE void publish(sfm_select_result* result, const sfm_select_result& r) const {
        __hip_atomic_store(&result->key, r.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&result->best_h, r.best_h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&result->best_err, r.best_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&result->first_flagged, r.first_flagged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&result->n_flagged, r.n_flagged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&result->best_cnt, r.best_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ONE thread of a waiting block, SLEEP: the s_sleep argument between two polls (units of 64 clocks).  False: the flag did not
    // come up within the bound.
    template <int SLEEP>
    SFM_DEVICE bool await() const {
        int polls = 0;
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && polls < kMaxFlagPolls) {
            __builtin_amdgcn_s_sleep(SLEEP);
            ++polls;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        return polls < kMaxFlagPolls;
    }
};

}  // namespace sfmsel
