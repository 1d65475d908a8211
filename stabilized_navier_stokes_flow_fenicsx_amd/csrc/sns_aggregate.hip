// Aggregation of the fine level by operator strength ON THE DEVICE (amg_aggregation = 2): the identical map that sns_host.cpp's
// aggregate_strength (amg_aggregation = 1) builds from the same strength, with only that map (4 B per node) copied to the host.
//
// The host function is a greedy heavy-edge matching over a strict total order (weight descending, then (min id, max id)
// ascending).  Over a strict total order the greedy result equals LOCALLY-DOMINANT matching: match every pair (a, b) where b is
// a's best eligible partner and a is b's, and repeat.  Each step matches at least the heaviest pending edge, so it always makes
// progress; a step that matches nothing while edges are pending is a bug and ends the build with SNS_E_HIP.  For a fixed cluster
// the order of its candidates is (weight descending, other id ascending).  The stages:
//   k_agg_smax / k_agg_strong   the strong graph: s_ij <- max(s_ij, s_ji) (the transposed slot by binary search in the sorted row
//                               j), smax per owned node, strong when w > 0 and w >= STRENGTH_THETA x smax of i or of j; one fp32
//                               weight per block slot (0 = not strong) -- a max of fp32 values, exact in fp32
//   k_agg_count / k_agg_fill    contraction to clusters: per cluster its members' strong slots into other clusters, insertion-
//                               sorted by the other cluster (stable) and merged, the weights summed in fp64 in member / slot order.
//                               The sums hold at most 16 fp32 terms within a few binary orders of magnitude: exact, so they do not
//                               depend on the order and match the host's.  No float atomics anywhere
//   k_agg_best / k_agg_match / k_agg_dirty
//                               one matching step (pairwise rounds; size filter size_a + size_b <= max_agg) over the clusters
//                               whose best partner may have changed
//   k_agg_lead ... k_agg_merge  renumbering in the order of the clusters' smallest member: a cluster leads when it is unmatched or
//                               the smaller of its pair, an exclusive scan of the leader flags gives the new ids
//   k_agg_lbest / k_agg_laccept / k_agg_lcommit
//                               leftover singles join their strongest adjacent cluster of >= 2 members with room: the pending edge
//                               (s, c) is accepted when it is s's best pending edge and fewer than room_c pending edges at c are
//                               heavier -- the sequential b-matching's result
// A step is three launches; the host reads three 4-byte counters (pending, matched, next list) after it.  No grid-wide barrier, no
// persistent kernel.  A rank without owned rows launches nothing.
#include "sns_ctx.h"

namespace sns {

namespace {

constexpr int AGG_TPB = 256;
constexpr int SCAN_ITEMS = 4;                          // per thread: 1024 per block
constexpr int SCAN_BLOCK = AGG_TPB * SCAN_ITEMS;

inline unsigned agg_blocks(int64_t n) { return (unsigned)((n + AGG_TPB - 1) / AGG_TPB); }

// (w1, d1) before (w2, d2) in the matcher's order for a fixed cluster: heavier first, then the smaller other id
__device__ inline bool agg_before(double w1, int32_t d1, double w2, int32_t d2) { return w1 > w2 || (w1 == w2 && d1 < d2); }

__device__ inline float agg_sym(int32_t i, int32_t k, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                const float* __restrict__ s) {
    const int32_t j = colind[k];
    int32_t lo = rowptr[j], hi = rowptr[j + 1];
    const int32_t end = hi;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (colind[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    const float sji = (lo < end && colind[lo] == i) ? s[lo] : 0.0f;
    const float sij = s[k];
    return sij < sji ? sji : sij;
}

// ---- exclusive scan of int32 counts into int64 offsets out[0..n] (out[n] = total), three launches ---------------------------------
__device__ inline int64_t block_exclusive_scan(int64_t v, int64_t* lds, int64_t* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int off = 1; off < AGG_TPB; off <<= 1) {
        const int64_t add = t >= off ? lds[t - off] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const int64_t incl = lds[t];
    *total = lds[AGG_TPB - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(AGG_TPB) void k_scan_sums(int32_t n, const int32_t* __restrict__ in, int64_t* __restrict__ bsum) {
    __shared__ int64_t lds[AGG_TPB];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t v = 0;
    for (int q = 0; q < SCAN_ITEMS; ++q)
        if (base + q < n) v += in[base + q];
    int64_t tot;
    block_exclusive_scan(v, lds, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(AGG_TPB) void k_scan_top(int32_t nb, int64_t* __restrict__ bsum, int32_t n, int64_t* __restrict__ out) {
    __shared__ int64_t lds[AGG_TPB];
    int64_t carry = 0;
    for (int32_t b0 = 0; b0 < nb; b0 += AGG_TPB) {
        const int32_t b = b0 + (int32_t)threadIdx.x;
        const int64_t v = b < nb ? bsum[b] : 0;
        int64_t tot;
        const int64_t ex = block_exclusive_scan(v, lds, &tot);
        if (b < nb) bsum[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(AGG_TPB) void k_scan_apply(int32_t n, const int32_t* __restrict__ in, const int64_t* __restrict__ bsum,
                                                        int64_t* __restrict__ out) {
    __shared__ int64_t lds[AGG_TPB];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    int32_t v[SCAN_ITEMS];
    int64_t sum = 0;
    for (int q = 0; q < SCAN_ITEMS; ++q) {
        v[q] = base + q < n ? in[base + q] : 0;
        sum += v[q];
    }
    int64_t tot;
    int64_t run = bsum[blockIdx.x] + block_exclusive_scan(sum, lds, &tot);
    for (int q = 0; q < SCAN_ITEMS; ++q)
        if (base + q < n) {
            out[base + q] = run;
            run += v[q];
        }
}

// ---- the strong graph ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AGG_TPB) void k_agg_smax(int32_t n_act, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                      const float* __restrict__ s, float* __restrict__ smax) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i >= n_act) return;
    float m = 0.0f;
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = colind[k];
        if (j == i || j >= n_act) continue;
        const float w = agg_sym(i, k, rowptr, colind, s);
        m = m < w ? w : m;
    }
    smax[i] = m;
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_strong(int32_t n_act, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                        const float* __restrict__ s, const float* __restrict__ smax, float* __restrict__ sw) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i >= n_act) return;
    const double ti = policy::STRENGTH_THETA * (double)smax[i];
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = colind[k];
        float out = 0.0f;
        if (j != i && j < n_act) {
            const float w = agg_sym(i, k, rowptr, colind, s);
            const double wd = (double)w;
            if (wd > 0.0 && (wd >= ti || wd >= policy::STRENGTH_THETA * (double)smax[j])) out = w;
        }
        sw[k] = out;
    }
}

// ---- contraction to clusters: mem[moff[c] .. moff[c + 1]) = the members of cluster c, of[i] = cluster of node i ----------------
__global__ __launch_bounds__(AGG_TPB) void k_agg_count(int32_t ncl, const int64_t* __restrict__ moff, const int32_t* __restrict__ mem,
                                                       const int32_t* __restrict__ of, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ colind, const float* __restrict__ sw,
                                                       int32_t* __restrict__ cnt) {
    const int32_t c = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (c >= ncl) return;
    int32_t r = 0;
    for (int64_t q = moff[c]; q < moff[c + 1]; ++q) {
        const int32_t i = mem[q];
        for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            if (sw[k] > 0.0f && of[colind[k]] != c) ++r;
    }
    cnt[c] = r;
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_fill(int32_t ncl, const int64_t* __restrict__ moff, const int32_t* __restrict__ mem,
                                                      const int32_t* __restrict__ of, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ colind, const float* __restrict__ sw,
                                                      const int64_t* __restrict__ eoff, int32_t* __restrict__ nbr,
                                                      double* __restrict__ wgt, int32_t* __restrict__ ecnt) {
    const int32_t c = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (c >= ncl) return;
    const int64_t e0 = eoff[c];
    int32_t m = 0;
    for (int64_t q = moff[c]; q < moff[c + 1]; ++q) {
        const int32_t i = mem[q];
        for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const float w = sw[k];
            const int32_t d = w > 0.0f ? of[colind[k]] : c;
            if (d == c) continue;
            // stable insertion by d: the entries of one d keep member / slot order
            int32_t p = m;
            while (p > 0 && nbr[e0 + p - 1] > d) {
                nbr[e0 + p] = nbr[e0 + p - 1];
                wgt[e0 + p] = wgt[e0 + p - 1];
                --p;
            }
            nbr[e0 + p] = d;
            wgt[e0 + p] = (double)w;
            ++m;
        }
    }
    int32_t u = 0;
    for (int32_t p = 0; p < m; ++p) {
        const int32_t d = nbr[e0 + p];
        const double w = wgt[e0 + p];
        if (u > 0 && nbr[e0 + u - 1] == d) {
            wgt[e0 + u - 1] += w;
        } else {
            nbr[e0 + u] = d;
            wgt[e0 + u] = w;
            ++u;
        }
    }
    ecnt[c] = u;
}

// ---- pairwise rounds ---------------------------------------------------------------------------------------------------------------
// A cluster's best eligible partner changes only when that partner is matched: eligibility only shrinks and the order is fixed.
// So a step recomputes `best` for the DIRTY clusters alone -- every cluster in a round's first step, then the unmatched clusters
// whose best was matched in the step before -- and every new mutual pair has a dirty member.  A dirty cluster with an eligible
// edge therefore means a match in the same step, and a step without dirty clusters with eligible edges ends the round.
// ctr[0] = dirty clusters with an eligible edge, ctr[1] = clusters matched in this step (listed in `matched`), ctr[2] = the next
// step's dirty clusters (listed in `next`; the order of a list does not matter, its members' work is independent)
__global__ __launch_bounds__(AGG_TPB) void k_agg_best(int32_t nlist, const int32_t* __restrict__ list, int32_t mark, int max_agg,
                                                      const int64_t* __restrict__ eoff, const int32_t* __restrict__ ecnt,
                                                      const int32_t* __restrict__ nbr, const double* __restrict__ wgt,
                                                      const int32_t* __restrict__ size, const int32_t* __restrict__ partner,
                                                      int32_t* __restrict__ best, int32_t* __restrict__ dirty, int32_t* __restrict__ ctr) {
    const int32_t t = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (t >= nlist) return;
    const int32_t c = list[t];
    const int32_t sc = size[c];
    const int64_t e0 = eoff[c];
    int32_t b = -1;
    double bw = 0.0;
    for (int32_t p = 0; p < ecnt[c]; ++p) {
        const int32_t d = nbr[e0 + p];
        if (partner[d] >= 0 || sc + size[d] > max_agg) continue;
        const double w = wgt[e0 + p];
        if (b < 0 || agg_before(w, d, bw, b)) { b = d; bw = w; }
    }
    best[c] = b;
    dirty[c] = mark;
    if (b >= 0) atomicAdd(&ctr[0], 1);
}

// a mutual pair (c, d) is taken by c when d is not dirty (its best is older and already c) or when c is the smaller of the two
__global__ __launch_bounds__(AGG_TPB) void k_agg_match(int32_t nlist, const int32_t* __restrict__ list, int32_t mark,
                                                       const int32_t* __restrict__ best, const int32_t* __restrict__ dirty,
                                                       int32_t* __restrict__ partner, int32_t* __restrict__ matched, int32_t* __restrict__ ctr) {
    const int32_t t = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (t >= nlist) return;
    const int32_t c = list[t];
    const int32_t d = best[c];
    if (d >= 0 && best[d] == c && (dirty[d] != mark || c < d)) {
        partner[c] = d;
        partner[d] = c;
        const int32_t q = atomicAdd(&ctr[1], 2);
        matched[q] = c;
        matched[q + 1] = d;
    }
}

// the next step's dirty clusters: unmatched neighbours of a newly matched cluster whose best it was
__global__ __launch_bounds__(AGG_TPB) void k_agg_dirty(int32_t nmax, const int32_t* __restrict__ matched, const int64_t* __restrict__ eoff,
                                                       const int32_t* __restrict__ ecnt, const int32_t* __restrict__ nbr,
                                                       const int32_t* __restrict__ best, const int32_t* __restrict__ partner,
                                                       int32_t* __restrict__ next, int32_t* __restrict__ ctr) {
    const int32_t t = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (t >= nmax || t >= ctr[1]) return;
    const int32_t m = matched[t];
    const int64_t e0 = eoff[m];
    for (int32_t p = 0; p < ecnt[m]; ++p) {
        const int32_t x = nbr[e0 + p];
        if (partner[x] < 0 && best[x] == m) next[atomicAdd(&ctr[2], 1)] = x;
    }
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_seq(int32_t n, int32_t* __restrict__ list) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i < n) list[i] = i;
}

// leader flags: unmatched, or the smaller of its pair
__global__ __launch_bounds__(AGG_TPB) void k_agg_lead(int32_t ncl, const int32_t* __restrict__ partner, int32_t* __restrict__ lead) {
    const int32_t c = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (c >= ncl) return;
    const int32_t p = partner[c];
    lead[c] = (p < 0 || c < p) ? 1 : 0;
}

// new id and size of every leader's merged cluster
__global__ __launch_bounds__(AGG_TPB) void k_agg_newid(int32_t ncl, const int32_t* __restrict__ partner, const int32_t* __restrict__ lead,
                                                       const int64_t* __restrict__ scan, const int32_t* __restrict__ size,
                                                       int32_t* __restrict__ newid, int32_t* __restrict__ nsize) {
    const int32_t c = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (c >= ncl) return;
    const int32_t p = partner[c];
    newid[c] = (int32_t)(lead[c] ? scan[c] : scan[p]);
    if (lead[c]) nsize[scan[c]] = size[c] + (p >= 0 ? size[p] : 0);
}

// member lists of the new clusters (the leader's members, then its partner's) at nmoff[new id]
__global__ __launch_bounds__(AGG_TPB) void k_agg_merge(int32_t ncl, const int32_t* __restrict__ partner, const int32_t* __restrict__ lead,
                                                       const int32_t* __restrict__ newid, const int64_t* __restrict__ moff,
                                                       const int32_t* __restrict__ mem, const int64_t* __restrict__ nmoff,
                                                       int32_t* __restrict__ nmem) {
    const int32_t c = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (c >= ncl || !lead[c]) return;
    int64_t o = nmoff[newid[c]];
    for (int64_t q = moff[c]; q < moff[c + 1]; ++q) nmem[o++] = mem[q];
    const int32_t p = partner[c];
    if (p >= 0)
        for (int64_t q = moff[p]; q < moff[p + 1]; ++q) nmem[o++] = mem[q];
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_relabel(int32_t n_act, const int32_t* __restrict__ newid, int32_t* __restrict__ of) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i < n_act) of[i] = newid[of[i]];
}

// ---- leftover singles --------------------------------------------------------------------------------------------------------------
// (s, c) is pending while s is a single without target and c has >= 2 members and room (max_agg - size - fill > 0)
__global__ __launch_bounds__(AGG_TPB) void k_agg_lbest(int32_t ncl, int max_agg, const int64_t* __restrict__ eoff, const int32_t* __restrict__ ecnt,
                                                       const int32_t* __restrict__ nbr, const double* __restrict__ wgt,
                                                       const int32_t* __restrict__ size, const int32_t* __restrict__ fill,
                                                       const int32_t* __restrict__ target, int32_t* __restrict__ best,
                                                       double* __restrict__ bestw, int32_t* __restrict__ ctr) {
    const int32_t x = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (x >= ncl) return;
    int32_t b = -1;
    double bw = 0.0;
    if (size[x] == 1 && target[x] < 0) {
        const int64_t e0 = eoff[x];
        for (int32_t p = 0; p < ecnt[x]; ++p) {
            const int32_t d = nbr[e0 + p];
            if (size[d] < 2 || max_agg - size[d] - fill[d] <= 0) continue;
            const double w = wgt[e0 + p];
            if (b < 0 || agg_before(w, d, bw, b)) { b = d; bw = w; }
        }
    }
    best[x] = b;
    bestw[x] = bw;
    if (b >= 0) atomicAdd(&ctr[0], 1);
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_laccept(int32_t ncl, int max_agg, const int64_t* __restrict__ eoff, const int32_t* __restrict__ ecnt,
                                                         const int32_t* __restrict__ nbr, const double* __restrict__ wgt,
                                                         const int32_t* __restrict__ size, const int32_t* __restrict__ fill,
                                                         const int32_t* __restrict__ target, const int32_t* __restrict__ best,
                                                         const double* __restrict__ bestw, int32_t* __restrict__ choose,
                                                         int32_t* __restrict__ ctr) {
    const int32_t x = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (x >= ncl) return;
    const int32_t c = best[x];
    int32_t out = -1;
    if (c >= 0) {
        const double wx = bestw[x];
        const int32_t room = max_agg - size[c] - fill[c];
        const int64_t e0 = eoff[c];
        int32_t heavier = 0;
        for (int32_t p = 0; p < ecnt[c] && heavier < room; ++p) {
            const int32_t s = nbr[e0 + p];
            if (size[s] != 1 || target[s] >= 0) continue;
            if (agg_before(wgt[e0 + p], s, wx, x)) ++heavier;
        }
        if (heavier < room) {
            out = c;
            atomicAdd(&ctr[1], 1);
        }
    }
    choose[x] = out;
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_lcommit(int32_t ncl, const int32_t* __restrict__ choose, int32_t* __restrict__ target,
                                                         int32_t* __restrict__ fill) {
    const int32_t x = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (x >= ncl) return;
    const int32_t c = choose[x];
    if (c >= 0) {
        target[x] = c;
        atomicAdd(&fill[c], 1);
    }
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_keep(int32_t ncl, const int32_t* __restrict__ target, int32_t* __restrict__ keep) {
    const int32_t x = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (x < ncl) keep[x] = target[x] < 0 ? 1 : 0;
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_final(int32_t n, int32_t n_act, const int32_t* __restrict__ of, const int32_t* __restrict__ target,
                                                       const int64_t* __restrict__ scan, int32_t* __restrict__ agg) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i >= n) return;
    int32_t a = -1;
    if (i < n_act) {
        const int32_t c = of[i];
        const int32_t t = target[c];
        a = (int32_t)scan[t >= 0 ? t : c];
    }
    agg[i] = a;
}

__global__ __launch_bounds__(AGG_TPB) void k_agg_iota(int32_t n, int32_t* __restrict__ a, int32_t* __restrict__ b, int32_t* __restrict__ one) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i >= n) return;
    a[i] = i;
    b[i] = i;
    one[i] = 1;
}

// ---- the hybrid (amg_aggregation = 3): geometric aggregates re-matched where they cut a dominant coupling ----------------------
// gsize[a] <- members of geometric aggregate a (integer atomics: the counts do not depend on the order)
__global__ __launch_bounds__(AGG_TPB) void k_hyb_size(int32_t n_act, const int32_t* __restrict__ g, int32_t* __restrict__ gsize) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i < n_act) atomicAdd(&gsize[g[i]], 1);
}

// one lane per owned row: cut = the strongest symmetrised coupling to an owned node of another geometric aggregate, ref = the
// strongest inside its own or the row's mean over its owned neighbours (summed in fp64 in slot order), whichever is larger -- the
// mean alone for a singleton; cut > HYBRID_KAPPA x ref marks the row, which dissolves its aggregate (every writer stores the same 1)
__global__ __launch_bounds__(AGG_TPB) void k_hyb_mark(int32_t n_act, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                      const float* __restrict__ s, const int32_t* __restrict__ g,
                                                      const int32_t* __restrict__ gsize, double kappa, int32_t* __restrict__ dis,
                                                      int32_t* __restrict__ nmark) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i >= n_act) return;
    const int32_t gi = g[i];
    float cut = 0.0f, kept = 0.0f;
    double sum = 0.0;
    int32_t cnt = 0;
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = colind[k];
        if (j == i || j >= n_act) continue;
        const float w = agg_sym(i, k, rowptr, colind, s);
        sum += (double)w;
        ++cnt;
        if (g[j] == gi) kept = kept < w ? w : kept;
        else cut = cut < w ? w : cut;
    }
    const double mean = cnt > 0 ? sum / (double)cnt : 0.0;
    const double ref = gsize[gi] == 1 ? mean : fmax((double)kept, mean);
    if ((double)cut > kappa * ref) {
        dis[gi] = 1;
        atomicAdd(nmark, 1);
    }
}

// inF[i] <- node i lies in a dissolved aggregate; keep[a] <- aggregate a is kept (all = 1: everything is dissolved)
__global__ __launch_bounds__(AGG_TPB) void k_hyb_flags(int32_t n_act, int32_t ng, int32_t all, const int32_t* __restrict__ g,
                                                       const int32_t* __restrict__ dis, int32_t* __restrict__ inF, int32_t* __restrict__ keep) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i < n_act) inF[i] = all ? 1 : dis[g[i]];
    if (i < ng) keep[i] = all ? 0 : 1 - dis[i];
}

// the induced subgraph of F: its rows in increasing node order (fnode[fpos[i]] = i) and per row the slots into F
__global__ __launch_bounds__(AGG_TPB) void k_hyb_count(int32_t n_act, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                       const int32_t* __restrict__ inF, const int64_t* __restrict__ fpos,
                                                       int32_t* __restrict__ fnode, int32_t* __restrict__ cnt) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i >= n_act || !inF[i]) return;
    int32_t c = 0;
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = colind[k];
        if (j < n_act && inF[j]) ++c;
    }
    const int64_t r = fpos[i];
    fnode[r] = i;
    cnt[r] = c;
}

// the subgraph's rows (the columns renumbered by fpos: increasing, so each row stays sorted) and the raw strength of its slots
__global__ __launch_bounds__(AGG_TPB) void k_hyb_fill(int32_t nF, const int32_t* __restrict__ fnode, int32_t n_act,
                                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                      const float* __restrict__ s, const int32_t* __restrict__ inF,
                                                      const int64_t* __restrict__ fpos, const int64_t* __restrict__ soff,
                                                      int32_t* __restrict__ srowptr, int32_t* __restrict__ scolind, float* __restrict__ ss) {
    const int32_t r = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (r >= nF) return;
    const int32_t i = fnode[r];
    int64_t p = soff[r];
    srowptr[r] = (int32_t)p;
    if (r == nF - 1) srowptr[nF] = (int32_t)soff[nF];
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = colind[k];
        if (j < n_act && inF[j]) {
            scolind[p] = (int32_t)fpos[j];
            ss[p] = s[k];
            ++p;
        }
    }
}

// the final map: kept geometric aggregates first, in order of their old ids (kpos), then F's aggregates (nkept = kpos[ng] + the
// subgraph's id); -1 for the ghosts
__global__ __launch_bounds__(AGG_TPB) void k_hyb_merge(int32_t n, int32_t n_act, int32_t ng, const int32_t* __restrict__ g,
                                                       const int32_t* __restrict__ inF, const int64_t* __restrict__ fpos,
                                                       const int64_t* __restrict__ kpos, const int32_t* __restrict__ sagg,
                                                       int32_t* __restrict__ agg) {
    const int32_t i = (int32_t)((int64_t)blockIdx.x * AGG_TPB + threadIdx.x);
    if (i >= n) return;
    int32_t a = -1;
    if (i < n_act) a = inF[i] ? (int32_t)kpos[ng] + sagg[fpos[i]] : (int32_t)kpos[g[i]];
    agg[i] = a;
}

struct Scanner {
    sns_ctx* h;
    int64_t* bsum;
    // out[0..n] <- exclusive scan of in[0..n), out[n] = total
    int run(const int32_t* in, int32_t n, int64_t* out) {
        const int32_t nb = (int32_t)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
        if (nb > 0) hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(AGG_TPB), 0, h->stream, n, in, bsum);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(AGG_TPB), 0, h->stream, nb, bsum, n, out);
        if (nb > 0) hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(AGG_TPB), 0, h->stream, n, in, bsum, out);
        HIP_TRY(hipGetLastError());
        return SNS_OK;
    }
};

template <class T>
int read_back(sns_ctx* h, const T* src, T* dst, size_t count) {
    HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SNS_OK;
}

// The strong graph and the matching over a graph VIEW: rows [0, n) of (rowptr, colind) -- sorted columns, so that the transposed
// slot is found by binary search -- of which the first n_act are aggregated; level 0 of the handle (amg_aggregation = 2) or the
// induced subgraph of the hybrid's dissolved aggregates (3).  `who` names the option in the error messages.
struct GraphView {
    const int32_t* rowptr;
    const int32_t* colind;
    int32_t n, n_act;
};

// sw[nnz of G] <- the strong-slot weights of G from its raw strength s (0: not strong); smax is scratch
int strong_slots(sns_ctx* h, const GraphView& G, const float* s, float* smax, float* sw) {
    if (G.n_act <= 0) return SNS_OK;
    hipLaunchKernelGGL(k_agg_smax, dim3(agg_blocks(G.n_act)), dim3(AGG_TPB), 0, h->stream, G.n_act, G.rowptr, G.colind, s, smax);
    hipLaunchKernelGGL(k_agg_strong, dim3(agg_blocks(G.n_act)), dim3(AGG_TPB), 0, h->stream, G.n_act, G.rowptr, G.colind, s, smax, sw);
    HIP_TRY(hipGetLastError());
    return SNS_OK;
}

// agg_dev[G.n] <- the map of aggregate_strength over G's first n_act nodes (-1 beyond), nc = aggregates; sw = strong_slots' weights
int match_strong(sns_ctx* h, const GraphView& G, const float* sw, int max_agg, const std::string& who, int32_t* agg_dev,
                 int32_t& nc) {
    const int32_t n = G.n, n_act = G.n_act;
    nc = 0;
    if (n_act <= 0) {
        if (n > 0) HIP_TRY(hipMemsetAsync(agg_dev, 0xff, (size_t)n * sizeof(int32_t), h->stream));
        return SNS_OK;
    }
    const size_t na = (size_t)n_act;
    // (device scratch, freed on every way out)
    DevBuf<int32_t> of, mem, nmem, size, nsize, partner, best, flag, newid, cnt, ecnt, nbr, ctr, fill, target, choose, list, next, dirty, matched;
    DevBuf<int64_t> moff, nmoff, eoff, scan, bsum;
    DevBuf<double> wgt, bestw;
    SNS_TRY(of.alloc(na));
    SNS_TRY(mem.alloc(na));
    SNS_TRY(nmem.alloc(na));
    SNS_TRY(size.alloc(na));
    SNS_TRY(nsize.alloc(na));
    SNS_TRY(partner.alloc(na));
    SNS_TRY(best.alloc(na));
    SNS_TRY(flag.alloc(na));
    SNS_TRY(newid.alloc(na));
    SNS_TRY(cnt.alloc(na));
    SNS_TRY(ecnt.alloc(na));
    SNS_TRY(fill.alloc(na));
    SNS_TRY(target.alloc(na));
    SNS_TRY(choose.alloc(na));
    SNS_TRY(bestw.alloc(na));
    SNS_TRY(list.alloc(na));
    SNS_TRY(next.alloc(na));
    SNS_TRY(dirty.alloc(na));
    SNS_TRY(matched.alloc(na));
    SNS_TRY(ctr.alloc(3));
    SNS_TRY(moff.alloc(na + 1));
    SNS_TRY(nmoff.alloc(na + 1));
    SNS_TRY(eoff.alloc(na + 1));
    SNS_TRY(scan.alloc(na + 1));
    SNS_TRY(bsum.alloc(na / SCAN_BLOCK + 1));
    Scanner scanner{h, bsum};
    const hipStream_t st = h->stream;
    // every node its own cluster: of = mem = identity, size 1, moff = 0, 1, 2, ...
    hipLaunchKernelGGL(k_agg_iota, dim3(agg_blocks(n_act)), dim3(AGG_TPB), 0, st, n_act, of, mem, size);
    SNS_TRY(scanner.run(size, n_act, moff));
    // the strong directed slots bound every contraction's entries
    int64_t cap = 0;
    {
        hipLaunchKernelGGL(k_agg_count, dim3(agg_blocks(n_act)), dim3(AGG_TPB), 0, st, n_act, moff, mem, of, G.rowptr, G.colind, sw, cnt);
        SNS_TRY(scanner.run(cnt, n_act, eoff));
        SNS_TRY(read_back(h, eoff + n_act, &cap, 1));
    }
    SNS_TRY(nbr.alloc((size_t)std::max<int64_t>(cap, 1)));
    SNS_TRY(wgt.alloc((size_t)std::max<int64_t>(cap, 1)));
    int32_t ncl = n_act;
    // contraction of the strong graph to the current clusters: (nbr, wgt)[eoff[c] .. + ecnt[c]) per cluster
    auto contract = [&]() -> int {
        hipLaunchKernelGGL(k_agg_count, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, moff, mem, of, G.rowptr, G.colind, sw, cnt);
        SNS_TRY(scanner.run(cnt, ncl, eoff));
        int64_t tot = 0;
        SNS_TRY(read_back(h, eoff + ncl, &tot, 1));
        if (tot > cap) { set_error(who + ": contraction exceeds the strong edges"); return SNS_E_HIP; }
        hipLaunchKernelGGL(k_agg_fill, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, moff, mem, of, G.rowptr, G.colind, sw, eoff,
                           nbr, wgt, ecnt);
        HIP_TRY(hipGetLastError());
        return SNS_OK;
    };
    for (int round = 1; (1 << round) <= max_agg; ++round) {
        SNS_TRY(contract());
        HIP_TRY(hipMemsetAsync(partner, 0xff, (size_t)ncl * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(dirty, 0, (size_t)ncl * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_agg_seq, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, list);
        // locally-dominant matching steps; each productive step matches at least one pair
        int32_t nlist = ncl;
        for (int32_t step = 0;; ++step) {
            if (step > ncl / 2 + 1) { set_error(who + ": matching did not finish"); return SNS_E_HIP; }
            const int32_t mark = step + 1, nmax = (int32_t)std::min<int64_t>(2 * (int64_t)nlist, ncl);
            HIP_TRY(hipMemsetAsync(ctr, 0, 3 * sizeof(int32_t), st));
            hipLaunchKernelGGL(k_agg_best, dim3(agg_blocks(nlist)), dim3(AGG_TPB), 0, st, nlist, list, mark, max_agg, eoff, ecnt, nbr, wgt,
                               size, partner, best, dirty, ctr);
            hipLaunchKernelGGL(k_agg_match, dim3(agg_blocks(nlist)), dim3(AGG_TPB), 0, st, nlist, list, mark, best, dirty, partner, matched, ctr);
            hipLaunchKernelGGL(k_agg_dirty, dim3(agg_blocks(nmax)), dim3(AGG_TPB), 0, st, nmax, matched, eoff, ecnt, nbr, best, partner, next, ctr);
            HIP_TRY(hipGetLastError());
            int32_t c3[3] = {0, 0, 0};
            SNS_TRY(read_back(h, ctr.get(), c3, 3));
            if (c3[0] == 0) break;                              // no eligible edge left anywhere
            if (c3[1] == 0) {
                set_error(who + ": a matching step matched nothing with " + std::to_string(c3[0]) + " clusters pending");
                return SNS_E_HIP;
            }
            std::swap(list, next);
            nlist = c3[2];
            if (nlist == 0) break;                              // every best is current and no pair is mutual: none left
        }
        // renumber in the order of the clusters' smallest member
        hipLaunchKernelGGL(k_agg_lead, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, partner, flag);
        SNS_TRY(scanner.run(flag, ncl, scan));
        int64_t nnew = 0;
        SNS_TRY(read_back(h, scan + ncl, &nnew, 1));
        hipLaunchKernelGGL(k_agg_newid, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, partner, flag, scan, size, newid, nsize);
        SNS_TRY(scanner.run(nsize, (int32_t)nnew, nmoff));
        hipLaunchKernelGGL(k_agg_merge, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, partner, flag, newid, moff, mem, nmoff, nmem);
        hipLaunchKernelGGL(k_agg_relabel, dim3(agg_blocks(n_act)), dim3(AGG_TPB), 0, st, n_act, newid, of);
        HIP_TRY(hipGetLastError());
        std::swap(mem, nmem);
        std::swap(moff, nmoff);
        std::swap(size, nsize);
        ncl = (int32_t)nnew;
    }
    // single nodes left over join their strongest adjacent cluster of at least two members that still has room
    SNS_TRY(contract());
    HIP_TRY(hipMemsetAsync(target, 0xff, (size_t)ncl * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(fill, 0, (size_t)ncl * sizeof(int32_t), st));
    for (int32_t step = 0;; ++step) {
        if (step > ncl + 1) { set_error(who + ": leftover assignment did not finish"); return SNS_E_HIP; }
        HIP_TRY(hipMemsetAsync(ctr, 0, 2 * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_agg_lbest, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, max_agg, eoff, ecnt, nbr, wgt, size, fill, target,
                           best, bestw, ctr);
        hipLaunchKernelGGL(k_agg_laccept, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, max_agg, eoff, ecnt, nbr, wgt, size, fill, target,
                           best, bestw, choose, ctr);
        hipLaunchKernelGGL(k_agg_lcommit, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, choose, target, fill);
        HIP_TRY(hipGetLastError());
        int32_t c2[2] = {0, 0};
        SNS_TRY(read_back(h, ctr.get(), c2, 2));
        if (c2[0] == 0) break;
        if (c2[1] == 0) {
            set_error(who + ": a leftover step accepted nothing with " + std::to_string(c2[0]) + " singles pending");
            return SNS_E_HIP;
        }
    }
    // the clusters without a target numbered in order; a targeted single takes its target's id
    hipLaunchKernelGGL(k_agg_keep, dim3(agg_blocks(ncl)), dim3(AGG_TPB), 0, st, ncl, target, flag);
    SNS_TRY(scanner.run(flag, ncl, scan));
    hipLaunchKernelGGL(k_agg_final, dim3(agg_blocks(n)), dim3(AGG_TPB), 0, st, n, n_act, of, target, scan, agg_dev);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    SNS_TRY(read_back(h, scan + ncl, &total, 1));
    nc = (int32_t)total;
    return SNS_OK;
}

}  // namespace

// agg[n] (host) <- the level-0 aggregation by operator strength of the owned nodes, built on the device; nc = aggregates.  The
// same map as aggregate_strength(level-0 pattern, n_owned, max_agg, strength).  Collective on a partitioned handle (the strength's
// halo exchange of the scales).
int aggregate_strength_device(sns_ctx* h, int max_agg, std::vector<int32_t>& agg, int32_t& nc) {
    const Level& L = h->levels[0];
    const int32_t n = L.n, n_act = h->n_owned;
    const GraphView G{L.rowptr, L.colind, n, n_act};
    agg.assign((size_t)n, -1);
    nc = 0;
    DevBuf<float> sw;                                               // strong-slot weights, one per block slot (0: not strong)
    {
        // the strength (collective) and the strong graph; the strength is freed again before the matching
        DevBuf<float> s, smax;
        DevBuf<double> scale;
        SNS_TRY(s.alloc((size_t)L.nnzb));
        SNS_TRY(scale.alloc(4 * (size_t)n));
        SNS_TRY(compute_strength(h, s, scale));
        if (n_act > 0) {
            SNS_TRY(smax.alloc((size_t)n_act));
            SNS_TRY(sw.alloc((size_t)L.nnzb));
        }
        if ((n_act > 0 && strong_slots(h, G, s, smax, sw) != SNS_OK) || hipStreamSynchronize(h->stream) != hipSuccess) {
            set_error("amg_aggregation = 2: strength or strong-graph kernel failed");
            return SNS_E_HIP;
        }
        if (n_act == 0) return SNS_OK;
    }
    DevBuf<int32_t> agg_dev;
    SNS_TRY(agg_dev.alloc((size_t)n));
    SNS_TRY(match_strong(h, G, sw, max_agg, "amg_aggregation = 2", agg_dev, nc));
    SNS_TRY(read_back(h, agg_dev.get(), agg.data(), (size_t)n));
    return SNS_OK;
}

// The hybrid (amg_aggregation = 3): agg[n] (host) <- the geometric map g of the owned nodes (ng aggregates, what amg_aggregation = 0
// builds) with every aggregate that cuts a dominant coupling dissolved and its nodes F re-matched by aggregate_strength on the
// induced subgraph of F (policy::HYBRID_KAPPA; everything when more than policy::HYBRID_PHI of the rows are marked: the map of
// amg_aggregation = 2); `rematched` = F is not empty on this rank.  When it is empty nothing runs after the mark step and the
// map is g itself.  Collective on a partitioned handle (the strength's halo exchange of the scales).
int aggregate_hybrid_device(sns_ctx* h, int max_agg, const std::vector<int32_t>& g, int32_t ng, std::vector<int32_t>& agg, int32_t& nc,
                            bool& rematched) {
    const Level& L = h->levels[0];
    const int32_t n = L.n, n_act = h->n_owned;
    const std::string who = "amg_aggregation = 3";
    agg = g;
    nc = ng;
    rematched = false;
    for (int32_t i = 0; i < n_act; ++i)
        if (g[(size_t)i] < 0 || g[(size_t)i] >= ng) { set_error(who + ": the geometric map is not total over the owned nodes"); return SNS_E_STATE; }
    // the fp32 strength: freed as soon as the subgraph holds the slots it needs (before the matching, as amg_aggregation = 2 does)
    DevBuf<float> s;
    {
        DevBuf<double> scale;
        SNS_TRY(s.alloc((size_t)L.nnzb));
        SNS_TRY(scale.alloc(4 * (size_t)n));
        SNS_TRY(compute_strength(h, s, scale));
    }
    if (n_act == 0) return SNS_OK;
    const hipStream_t st = h->stream;
    const size_t na = (size_t)n_act, nga = (size_t)std::max(1, ng);
    DevBuf<int32_t> d_g, gsize, dis, inF, keep, nmark;
    DevBuf<int64_t> fpos, kpos, bsum;
    SNS_TRY(d_g.alloc(na));
    SNS_TRY(gsize.alloc(nga));
    SNS_TRY(dis.alloc(nga));
    SNS_TRY(inF.alloc(na));
    SNS_TRY(keep.alloc(nga));
    SNS_TRY(nmark.alloc(1));
    SNS_TRY(fpos.alloc(na + 1));
    SNS_TRY(kpos.alloc(nga + 1));
    SNS_TRY(bsum.alloc(std::max(na, nga) / SCAN_BLOCK + 1));
    Scanner scanner{h, bsum};
    HIP_TRY(hipMemcpyAsync(d_g, g.data(), na * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(gsize, 0, nga * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(dis, 0, nga * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(nmark, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_hyb_size, dim3(agg_blocks(n_act)), dim3(AGG_TPB), 0, st, n_act, d_g, gsize);
    hipLaunchKernelGGL(k_hyb_mark, dim3(agg_blocks(n_act)), dim3(AGG_TPB), 0, st, n_act, L.rowptr, L.colind, s, d_g, gsize,
                       policy::HYBRID_KAPPA, dis, nmark);
    HIP_TRY(hipGetLastError());
    int32_t marked = 0;
    SNS_TRY(read_back(h, nmark.get(), &marked, 1));
    if (marked == 0) return SNS_OK;                                 // nothing dissolved: the geometric map
    // more than HYBRID_PHI of the rows marked: everything dissolved (the map of amg_aggregation = 2)
    const int32_t all = (double)marked > policy::HYBRID_PHI * (double)n_act ? 1 : 0;
    hipLaunchKernelGGL(k_hyb_flags, dim3(agg_blocks(std::max(n_act, ng))), dim3(AGG_TPB), 0, st, n_act, ng, all, d_g, dis, inF, keep);
    HIP_TRY(hipGetLastError());
    SNS_TRY(scanner.run(inF, n_act, fpos));
    int64_t nF = 0;
    SNS_TRY(read_back(h, fpos + n_act, &nF, 1));
    if (nF == 0) { set_error(who + ": marked rows without a dissolved aggregate"); return SNS_E_HIP; }
    const int32_t nf = (int32_t)nF;
    SNS_TRY(scanner.run(keep, ng, kpos));
    DevBuf<int32_t> fnode, cnt, srowptr, scolind, sagg, agg_dev;
    DevBuf<int64_t> soff;
    DevBuf<float> ss, smax, sw;
    SNS_TRY(fnode.alloc((size_t)nf));
    SNS_TRY(cnt.alloc((size_t)nf));
    SNS_TRY(soff.alloc((size_t)nf + 1));
    SNS_TRY(srowptr.alloc((size_t)nf + 1));
    hipLaunchKernelGGL(k_hyb_count, dim3(agg_blocks(n_act)), dim3(AGG_TPB), 0, st, n_act, L.rowptr, L.colind, inF, fpos, fnode, cnt);
    HIP_TRY(hipGetLastError());
    SNS_TRY(scanner.run(cnt, nf, soff));
    int64_t nnz = 0;
    SNS_TRY(read_back(h, soff + nf, &nnz, 1));
    if (nnz > (int64_t)L.nnzb) { set_error(who + ": the induced subgraph exceeds the pattern"); return SNS_E_HIP; }
    const size_t nz = (size_t)std::max<int64_t>(nnz, 1);
    SNS_TRY(scolind.alloc(nz));
    SNS_TRY(ss.alloc(nz));
    hipLaunchKernelGGL(k_hyb_fill, dim3(agg_blocks(nf)), dim3(AGG_TPB), 0, st, nf, fnode, n_act, L.rowptr, L.colind, s, inF, fpos, soff,
                       srowptr, scolind, ss);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    s.reset();
    SNS_TRY(sw.alloc(nz));
    SNS_TRY(smax.alloc((size_t)nf));
    SNS_TRY(sagg.alloc((size_t)nf));
    SNS_TRY(agg_dev.alloc((size_t)std::max(1, n)));
    // the matching of amg_aggregation = 2, unchanged, on the subgraph
    const GraphView G{srowptr, scolind, nf, nf};
    SNS_TRY(strong_slots(h, G, ss, smax, sw));
    int32_t snc = 0;
    SNS_TRY(match_strong(h, G, sw, max_agg, who, sagg, snc));
    hipLaunchKernelGGL(k_hyb_merge, dim3(agg_blocks(n)), dim3(AGG_TPB), 0, st, n, n_act, ng, d_g, inF, fpos, kpos, sagg, agg_dev);
    HIP_TRY(hipGetLastError());
    int64_t nkept = 0;
    SNS_TRY(read_back(h, kpos + ng, &nkept, 1));
    SNS_TRY(read_back(h, agg_dev.get(), agg.data(), (size_t)n));
    nc = (int32_t)nkept + snc;
    rematched = true;
    return SNS_OK;
}

}  // namespace sns
