// mdk_profile.hip -- the count profile of two [S, n] count matrices: per sample and group of sites the depth histogram, the level
// histogram, the two sums and the largest depth (include/mdk_profile.h: md_stats_profile, md_stats_profile_limits).  The rule is
// mdk_profile_core.h's.  Part of libmdk_stats.so: mdk_qdiff.hip includes this file below mdk_moments.hip, so the calls live on the
// md_stats handle, its stream, its status word and its error text.
//
// One pass over 8 bytes a cell (int32) and one byte a site.  The work is cut into ITEMS: a band of t samples (1, 2 or 4) times a range of
// sites.  A workgroup (256 lanes) takes items blockIdx.x, blockIdx.x + gridDim.x, ...:
//   zero    the band's histograms in LDS, 32-bit words -- a range is below 2^32 sites --, t G (B + 1 + L) of them
//   count   a lane per site, striding the range by 256, two sites at a time so that both sites' loads are on their way before a cell is
//           counted: the site's group byte read once for the band, the 2 t entries read coalesced along n, each cell made one word by prof_cell, and one LDS atomic add that returns nothing for its depth bin and one for
//           its level bin.  A depth of B or more also raises the band's max word -- read first, so the atomic is issued only by a lane
//           that would raise it.  The two sums are kept per lane, sample and group in 32-bit registers, the group picked by selects,
//           over a SPAN of 32 sites a lane (32 entries below 2^26 stay below 2^31); behind a span a wavefront adds them up by shuffles
//           in 64 bits and its lane 0 adds them to the band's sums in LDS
//   flush   the non-zero bins alone are added to the int64 outputs with device-scope atomic adds; the highest non-zero bin below B
//           raises the max word, which an atomic max then takes to max_depth
// Integer sums and a maximum commute: the outputs do not depend on the items, their order or the grid.
// The hazard is real data: depths concentrate in a dozen bins and most levels fall in the first and the last, so the lanes of a
// wavefront meet on one LDS word and the atomic serialises.  A remedy was built and measured -- the level bins and the first 32 depth
// bins held in 2, 4 or 8 copies on neighbouring banks, a lane counting into copy (lane mod copies) and the flush adding them up --: within
// 2 % of this plain form either way at every S and G, so it is gone; what bounds the kernel is not the LDS.
// So is the default band: one sample.  Bands of 2 and 4 read the group bytes less often, but fewer workgroups fit a CU and a lane needs
// more registers: measured 15 to 40 % slower where there are groups and within 8 % either way where there are none.  They stay for the hook.
// A refusal goes into the status word by atomicMin as in k_qdiff.  Vector loads, stores and atomics, plain C++.
#include "mdk_profile_core.h"

#define PROF_WG 256
#define PROF_GRID_DEFAULT 2048
#define PROF_RANGE 8192                   // the least sites of an item by default: the zeroing and the flush of a band are a small part of it
#define PROF_SPAN_SITES 32                // a lane's sites between two folds of its 32-bit sums
#define PROF_SITES 2                      // ... and those it loads at a time
#define PROF_BAND_DEFAULT 1               // (measured against 2 and 4: DESIGN.md section 4)
#define PROF_LDS_MAX 163840               // what a workgroup can have

struct KProf {
    const void *m, *u; const uint8_t *group; int32_t S; int64_t n, min_depth; int32_t B, L;
    int32_t cw, sums_at;                                           // a (sample, group)'s words: B + 1 depth bins, then L level bins; where the band's sums start
    int64_t nranges, range, items;
    unsigned long long *dh, *lh, *ms, *us, *mx;
    StatsStatus *st;
};

extern __shared__ __align__(16) uint32_t prof_lds[];
__device__ __forceinline__ void prof_count(uint32_t *p) { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <typename T, int t, int G>
__global__ __launch_bounds__(PROF_WG) void k_profile(const KProf K) {
    const T *const __restrict__ M = (const T *)K.m, *const __restrict__ U = (const T *)K.u;
    const uint8_t *const __restrict__ group = K.group;
    const int lane = threadIdx.x & 63;
    const uint32_t cw = (uint32_t)K.cw, lvl = (uint32_t)K.B + 1u;
    uint32_t *const hist = prof_lds;
    unsigned long long *const sums = (unsigned long long *)(prof_lds + K.sums_at);          // [t G][2]: nmeth_sum, nunmeth_sum
    uint32_t *const maxw = prof_lds + K.sums_at + 4 * t * G;                                // [t G]
    const int32_t words = K.sums_at + 5 * t * G, logical = K.B + 1 + K.L;
    unsigned long long first = ~0ull;
    for(int64_t item = blockIdx.x; item < K.items; item += gridDim.x) {
        const int64_t band = item / K.nranges, r = item - band * K.nranges;
        const int32_t s0 = (int32_t)band * t;
        const int64_t k0 = r * K.range, k1 = k0 + K.range < K.n ? k0 + K.range : K.n;
        for(int32_t x = threadIdx.x; x < words; x += PROF_WG) prof_lds[x] = 0u;
        __syncthreads();
        for(int64_t span = k0; span < k1; span += (int64_t)PROF_SPAN_SITES * PROF_WG) {
            const int64_t e1 = span + (int64_t)PROF_SPAN_SITES * PROF_WG < k1 ? span + (int64_t)PROF_SPAN_SITES * PROF_WG : k1;
            uint32_t pm[t][G], pu[t][G];
#pragma unroll
            for(int a = 0; a < t; a++)
#pragma unroll
                for(int g = 0; g < G; g++) { pm[a][g] = 0u; pu[a][g] = 0u; }
            for(int64_t k = span + threadIdx.x; k < e1; k += PROF_SITES * PROF_WG) {
                // a lane's PROF_SITES sites, a workgroup's width apart: every load of them is on its way before the first cell is counted
                uint32_t gk[PROF_SITES]; int64_t m[PROF_SITES][t], u[PROF_SITES][t];
#pragma unroll
                for(int j = 0; j < PROF_SITES; j++) {
                    const int64_t kk = k + j * PROF_WG;
                    const bool on = kk < e1;
                    gk[j] = on && group ? (uint32_t)group[kk] : 0u;
#pragma unroll
                    for(int a = 0; a < t; a++) {
                        const int64_t at = (int64_t)(s0 + a) * K.n + kk;
                        const bool live = on && s0 + a < K.S;
                        m[j][a] = live ? (int64_t)M[at] : 0; u[j][a] = live ? (int64_t)U[at] : 0;
                    }
                }
#pragma unroll
                for(int j = 0; j < PROF_SITES; j++) {
                    const int64_t kk = k + j * PROF_WG;
                    if(kk >= e1) continue;
                    uint32_t err = prof_group_check(gk[j], G);
                    const bool site_ok = !err;
                    const uint32_t gs = site_ok ? gk[j] : 0u;
#pragma unroll
                    for(int a = 0; a < t; a++) {
                        if(s0 + a >= K.S) continue;                // (the same for every lane)
                        const uint32_t w = prof_cell(m[j][a], u[j][a], K.min_depth, K.B, K.L, &err);
                        if(w == PROF_REFUSED || !site_ok) continue;
                        const uint32_t ag = (uint32_t)a * G + gs, base = ag * cw, db = w & PROF_DEPTH_MASK;
                        prof_count(&hist[base + db]);
                        if(db == (uint32_t)K.B) {
                            const uint32_t d = (uint32_t)(m[j][a] + u[j][a]);              // (below 2^27)
                            if(d > *(volatile uint32_t *)&maxw[ag]) (void)__hip_atomic_fetch_max(&maxw[ag], d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        const bool covered = (w >> PROF_COVERED_BIT) & 1u;
                        if(covered) prof_count(&hist[base + lvl + (w >> 16)]);
                        const uint32_t mc = covered ? (uint32_t)m[j][a] : 0u, uc = covered ? (uint32_t)u[j][a] : 0u;
#pragma unroll
                        for(int g = 0; g < G; g++) { pm[a][g] += G == 1 || gs == (uint32_t)g ? mc : 0u; pu[a][g] += G == 1 || gs == (uint32_t)g ? uc : 0u; }
                    }
                    if(err) { const unsigned long long key = mom_refusal_key(kk, err); first = key < first ? key : first; }
                }
            }
            // the span's sums: a wavefront's on its lane 0, which adds them to the band's
#pragma unroll
            for(int a = 0; a < t; a++)
#pragma unroll
                for(int g = 0; g < G; g++) {
                    unsigned long long v[2] = { pm[a][g], pu[a][g] };
#pragma unroll
                    for(int q = 0; q < 2; q++) {
#pragma unroll
                        for(int off = 32; off; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
                        if(lane == 0 && v[q]) (void)__hip_atomic_fetch_add(&sums[(a * G + g) * 2 + q], v[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
        }
        __syncthreads();
        // the non-zero bins of the band, a (sample, group) after the other
        for(int32_t ag = 0; ag < t * G; ag++) {
            const int32_t a = ag / G, g = ag - a * G, s = s0 + a;
            if(s >= K.S) break;
            const uint32_t base = (uint32_t)ag * cw;
            const int64_t to = (int64_t)s * G + g;
            for(int32_t b = threadIdx.x; b < logical; b += PROF_WG) {
                const uint32_t v = hist[base + b];
                if(!v) continue;
                const bool depth = b <= K.B;
                const uint32_t bin = depth ? (uint32_t)b : (uint32_t)b - lvl;
                if(depth) {
                    atomicAdd(K.dh + to * (K.B + 1) + bin, (unsigned long long)v);
                    if(b < K.B && bin > *(volatile uint32_t *)&maxw[ag]) (void)__hip_atomic_fetch_max(&maxw[ag], bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else atomicAdd(K.lh + to * K.L + bin, (unsigned long long)v);
            }
        }
        __syncthreads();
        if(threadIdx.x < t * G && s0 + (int32_t)threadIdx.x / G < K.S) {
            const int64_t to = (int64_t)(s0 + (int32_t)threadIdx.x / G) * G + (int32_t)threadIdx.x % G;
            const unsigned long long vm = sums[threadIdx.x * 2], vu = sums[threadIdx.x * 2 + 1], top = maxw[threadIdx.x];
            if(vm) atomicAdd(K.ms + to, vm);
            if(vu) atomicAdd(K.us + to, vu);
            if(top) atomicMax(K.mx + to, top);
        }
        __syncthreads();                                           // (the LDS is zeroed again for the next item)
    }
    if(first != ~0ull) atomicMin(&K.st->first, first);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int md_stats_profile_limits(md_stats *h, int32_t range_sites, int32_t band_samples, int32_t max_workgroups) {
    const char *const what = "md_stats_profile_limits";
    if(!h) return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    const bool band_ok = band_samples == 0 || band_samples == 1 || band_samples == 2 || band_samples == 4;
    if(range_sites < 0 || range_sites % 64 || range_sites > MOM_MAX_SITES || !band_ok || max_workgroups < 0) {
        snprintf(g_err, sizeof g_err, "%s: range_sites a multiple of 64 up to 2^30, band_samples 0, 1, 2 or 4, max_workgroups 0 or more", what);
        return MD_STATS_ERR_ARG;
    }
    h->prof_range = range_sites; h->prof_band = band_samples; h->prof_grid = max_workgroups;
    return 0;
}

// what a call launches at these limits: the kernel's arguments without its pointers
struct ProfPlan { int32_t band, grid; size_t lds; };
// the LDS words of a band of t samples, K's layout filled in
static size_t prof_words(int32_t t, int32_t G, int32_t B, int32_t L, KProf *K) {
    K->cw = B + 1 + L;
    K->sums_at = (t * G * K->cw + 1) / 2 * 2;                      // (the sums are 64-bit words)
    return (size_t)K->sums_at + 5 * (size_t)t * G;
}
static ProfPlan prof_plan(const md_stats *h, int32_t S, int64_t n, int32_t G, int32_t B, int32_t L, KProf *K) {
    ProfPlan p;
    p.band = h->prof_band ? h->prof_band : PROF_BAND_DEFAULT;
    while(p.band > 1 && (p.band / 2 >= S || prof_words(p.band, G, B, L, K) * 4 > PROF_LDS_MAX)) p.band /= 2;         // (one sample is 70 KB at the most)
    p.lds = prof_words(p.band, G, B, L, K) * 4;
    K->S = S; K->n = n; K->B = B; K->L = L;
    const int64_t nbands = (S + p.band - 1) / p.band, wanted = PROF_GRID_DEFAULT / nbands > 0 ? PROF_GRID_DEFAULT / nbands : 1;
    if(h->prof_range) K->range = h->prof_range;
    else {
        K->range = ((n + wanted - 1) / wanted + 63) / 64 * 64;
        if(K->range < PROF_RANGE) K->range = PROF_RANGE;
    }
    K->nranges = (n + K->range - 1) / K->range;
    K->items = nbands * K->nranges;
    const int64_t most = h->prof_grid ? h->prof_grid : PROF_GRID_DEFAULT;
    p.grid = (int32_t)(K->items < most ? K->items : most);
    return p;
}

template <typename T, int t, int G> static hipError_t prof_launch_one(const md_stats *h, const ProfPlan &p, const KProf &K) {
    if(p.lds > 65536) {                                            // (past what a launch may ask without saying so)
        const hipError_t e = hipFuncSetAttribute((const void *)k_profile<T, t, G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if(e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_profile<T, t, G>), dim3(p.grid), dim3(PROF_WG), p.lds, h->st, K);
    return hipGetLastError();
}
template <typename T, int t> static hipError_t prof_launch_band(const md_stats *h, const ProfPlan &p, const KProf &K, int32_t G) {
    return G == 1 ? prof_launch_one<T, t, 1>(h, p, K) : G == 2 ? prof_launch_one<T, t, 2>(h, p, K) : G == 3 ? prof_launch_one<T, t, 3>(h, p, K) : prof_launch_one<T, t, 4>(h, p, K);
}
template <typename T> static hipError_t prof_launch_as(const md_stats *h, const ProfPlan &p, const KProf &K, int32_t G) {
    return p.band == 1 ? prof_launch_band<T, 1>(h, p, K, G) : p.band == 2 ? prof_launch_band<T, 2>(h, p, K, G) : prof_launch_band<T, 4>(h, p, K, G);
}
static hipError_t prof_launch(const md_stats *h, const ProfPlan &p, const KProf &K, int32_t G, int elem_bytes) {
    return elem_bytes == 4 ? prof_launch_as<int32_t>(h, p, K, G) : prof_launch_as<int64_t>(h, p, K, G);
}

extern "C" int md_stats_profile(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                                const uint8_t *group, int32_t n_groups, int64_t min_depth, int32_t depth_bins, int32_t level_bins,
                                int64_t *depth_hist, int64_t *level_hist, int64_t *nmeth_sum, int64_t *nunmeth_sum, int64_t *max_depth) {
    const char *const what = "md_stats_profile";
    if(!h || (elem_bytes != 4 && elem_bytes != 8) || n_samples < 1 || n_samples > MOM_MAX_SAMPLES || n < 0 || n > MOM_MAX_SITES ||
       !depth_hist || !level_hist || !nmeth_sum || !nunmeth_sum || !max_depth)
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(n && (!nmeth || !nunmeth)) return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(min_depth < 1 || min_depth >= MOM_LIMIT) {
        snprintf(g_err, sizeof g_err, "%s: min_depth must be within 1 and 2^26 - 1", what);
        return MD_STATS_ERR_ARG;
    }
    if(n_groups < 1 || n_groups > PROF_MAX_GROUPS || depth_bins < 1 || depth_bins > PROF_MAX_DEPTH_BINS || level_bins < 1 || level_bins > PROF_MAX_LEVEL_BINS) {
        snprintf(g_err, sizeof g_err, "%s: n_groups must be within 1 and %d, depth_bins within 1 and %d, level_bins within 1 and %d", what, PROF_MAX_GROUPS, PROF_MAX_DEPTH_BINS, PROF_MAX_LEVEL_BINS);
        return MD_STATS_ERR_ARG;
    }
    SIDECHK(hipSetDevice(h->device));
    const size_t cells = (size_t)n_samples * n_groups;
    SIDECHK(hipMemsetAsync(depth_hist, 0, cells * (depth_bins + 1) * sizeof(int64_t), h->st)); SIDECHK(hipMemsetAsync(level_hist, 0, cells * level_bins * sizeof(int64_t), h->st));
    SIDECHK(hipMemsetAsync(nmeth_sum, 0, cells * sizeof(int64_t), h->st)); SIDECHK(hipMemsetAsync(nunmeth_sum, 0, cells * sizeof(int64_t), h->st));
    SIDECHK(hipMemsetAsync(max_depth, 0, cells * sizeof(int64_t), h->st));
    if(!n) { SIDECHK(hipStreamSynchronize(h->st)); return 0; }
    SIDE_STATUS_UP(h, &h->pin->st, StatsStatus);
    KProf K;
    K.m = nmeth; K.u = nunmeth; K.group = group; K.min_depth = min_depth; K.st = h->d_st;
    K.dh = (unsigned long long *)depth_hist; K.lh = (unsigned long long *)level_hist; K.ms = (unsigned long long *)nmeth_sum; K.us = (unsigned long long *)nunmeth_sum;
    K.mx = (unsigned long long *)max_depth;
    const ProfPlan p = prof_plan(h, n_samples, n, n_groups, depth_bins, level_bins, &K);
    SIDECHK(prof_launch(h, p, K, n_groups, elem_bytes));
    SIDE_STATUS_DOWN(h, &h->pin->st, StatsStatus);
    const unsigned long long first = h->pin->st.first;
    if(first == ~0ull) return 0;
    const uint32_t bit = 1u << (first & 0xffu);
    if(bit == PROF_E_GROUP) snprintf(g_err, sizeof g_err, "%s: a site's group is %d or more (site %lld)", what, (int)n_groups, (long long)(first >> 8));
    else snprintf(g_err, sizeof g_err, "%s: %s (site %lld)", what, bit == MOM_E_NEGATIVE ? "a count is negative" : "a count is 2^26 or more", (long long)(first >> 8));
    return MD_STATS_ERR_ARG;
}

// three or more groups of replicates: one more call and one more kernel of the library, on the same handle (this file is the last
// that mdk_qdiff.hip includes, and it hands on to the next)
#include "mdk_gdiff.hip"
