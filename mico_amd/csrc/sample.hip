// Sampling decode step on the device (include/mico_hip.h, "Device-side sampling"): logits processors, temperature, top-k and top-p warpers
// and one inverse-CDF draw per row, with the finished-row bookkeeping of the decode loop (mico_warp_sample).
#include "common.h"
#include <stddef.h>

namespace {

constexpr int SAMPLE_K_MAX = 64;                 // largest top_k: the kept candidates fit one wave, one lane per rank
constexpr int SAMPLE_BITMAP_V = 65536;           // largest vocabulary of the processors' two bitmaps (mico_beam_topk's)
constexpr int SAMPLE_IDS_MAX = 512;
constexpr int SAMPLE_STAGE_CHUNK = 136;          // columns per thread of a row that is staged in LDS: V <= 136 * 256 = 34816
constexpr int SAMPLE_STAGE_LD = 257;             // [chunk position][thread], padded: the fill and the passes are both conflict-free
constexpr unsigned KEY_NEG_INF = 0x007fffffu;    // score_key(-inf): every finite score's key is above it, NaN's (0) below

// A processed score as a 32-bit key, monotonic in the score (topk_key's high word): -0 -> +0, NaN lowest.
__device__ __forceinline__ unsigned score_key(float v) {
    v += 0.f;
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (v != v) u = 0u;
    return u;
}
__device__ __forceinline__ float key_score(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
// weight e^(s - m) of a key; no weight for -inf and NaN
__device__ __forceinline__ float key_weight(unsigned k, float m) { return k > KEY_NEG_INF ? __expf(key_score(k) - m) : 0.f; }

// Block reductions over the four waves through a double-buffered LDS slot: one barrier per reduction, every thread gets the result, and the
// order of the operations is fixed, so a sum is the same number in every run.
struct BlockRed {
    unsigned (*slot)[4];
    int phase, lane, wave;
    __device__ __forceinline__ void exchange(unsigned v, unsigned (&o)[4]) {
        if (lane == 0) slot[phase][wave] = v;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) o[w] = slot[phase][w];
        phase ^= 1;
    }
    __device__ __forceinline__ double sum(double v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        unsigned lo[4], hi[4];
        if (lane == 0) { slot[phase][wave] = (unsigned)b; slot[phase + 2][wave] = (unsigned)(b >> 32); }
        __syncthreads();
        double t[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            lo[w] = slot[phase][w];
            hi[w] = slot[phase + 2][w];
            t[w] = __longlong_as_double((long long)(((unsigned long long)hi[w] << 32) | lo[w]));
        }
        phase ^= 1;
        return ((t[0] + t[1]) + t[2]) + t[3];
    }
    __device__ __forceinline__ int sum(int v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        unsigned o[4];
        exchange((unsigned)v, o);
        return (int)(o[0] + o[1] + o[2] + o[3]);
    }
    __device__ __forceinline__ unsigned max(unsigned v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const unsigned t = __shfl_xor(v, d, 64); v = t > v ? t : v; }
        unsigned o[4];
        exchange(v, o);
        return ::max(::max(o[0], o[1]), ::max(o[2], o[3]));
    }
    __device__ __forceinline__ unsigned min(unsigned v) { return ~max(~v); }
};

// One 256-thread workgroup per row; thread t owns the contiguous columns [t chunk, (t + 1) chunk), chunk = ceil(V / 256), so a running sum in
// column order is (exclusive scan of the chunk sums) + (the chunk's own sequential sum), as in vocab_sample_kernel.  Every column's processed
// score s = processed(x) / temperature becomes a 32-bit monotonic key.  STAGED: the keys are computed once and kept in LDS (one workgroup per
// CU); otherwise every pass recomputes them from the row in L2.  The cut of both warpers is one bitwise binary search over the key, 32 passes
// of one block reduction each:
//   top-k: the largest key f with count(key >= f) >= k (an integer count), then the columns above f and the first of the columns equal to f;
//   top-p (top_k = 0): the largest key f with mass(key > f) >= top_p * total, the kept set being key > f.  mass() and total are the same fixed
//   tree of additions, which is monotonic in its terms, so the predicate is monotonic in f and the search is exact for it.  The terms are the
//   fp32 weights e^(s - max); they are added in fp64 (full rate on this chip), so that where the boundary falls among columns of 1e-5 of the
//   mass each it is placed by the weights, not by the order of the additions - and the draw's running sum likewise.
// The top-k candidates (<= 64) are ranked by counting and handled by wave 0, lane r holding rank r: softmax, top-p over the ranks, the draw.
template <bool STAGED>
__global__ __launch_bounds__(256) void warp_sample_kernel(const mico_warp_sample_params p) {
    __shared__ unsigned s_stage[STAGED ? SAMPLE_STAGE_CHUNK * SAMPLE_STAGE_LD : 1];
    __shared__ unsigned s_seen[SAMPLE_BITMAP_V / 32], s_ban[SAMPLE_BITMAP_V / 32];
    __shared__ unsigned long long s_cand[SAMPLE_K_MAX];
    __shared__ unsigned s_red[4][4];      // two phases, low and high words
    __shared__ double s_scan[4];
    __shared__ int s_n;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = p.V, cur_len = p.cur_len;
    int64_t* rid = p.ids ? p.ids + (int64_t)row * p.ld_ids : nullptr;
    const bool appending = p.append != 0 && rid != nullptr;
    if (p.unfinished && !p.unfinished[row]) {      // (block-uniform) a finished row: pad
        if (tid == 0) {
            p.token[row] = p.pad_id;
            if (p.logp) p.logp[row] = 0.f;
            if (p.n_kept) p.n_kept[row] = 0;
            if (p.kept_min) p.kept_min[row] = 0.f;
            if (appending) rid[cur_len] = p.pad_id;
        }
        return;
    }
    const float* x = p.logits + (int64_t)row * p.ld;
    const float pen = p.rep_penalty, temp = p.temperature;
    const bool use_ids = rid != nullptr;
    BlockRed red{s_red, 0, lane, wave};

    if (use_ids) {      // the processors' bitmaps (beam_row_kernel's)
        for (int i = tid; i < (V + 31) / 32; i += 256) { s_seen[i] = 0u; s_ban[i] = 0u; }
        __syncthreads();
        if (pen != 1.f)
            for (int i = tid; i < cur_len; i += 256) {
                const int64_t t = rid[i];
                if (t >= 0 && t < V) atomicOr(&s_seen[t >> 5], 1u << (t & 31));
            }
        if (p.ngram > 0 && cur_len >= p.ngram) {
            const int ngram = p.ngram, nwin = cur_len - ngram + 1, tail = cur_len - ngram + 1;
            for (int i = tid; i < nwin; i += 256) {
                bool match = true;
                for (int q = 0; q < ngram - 1; ++q) match = match && rid[i + q] == rid[tail + q];
                const int64_t t = rid[i + ngram - 1];
                if (match && t >= 0 && t < V) atomicOr(&s_ban[t >> 5], 1u << (t & 31));
            }
        }
        if (p.ban_eos && tid == 0 && p.eos_id >= 0 && p.eos_id < V) atomicOr(&s_ban[p.eos_id >> 5], 1u << (p.eos_id & 31));
        __syncthreads();
    }
    auto column_key = [&](int j) -> unsigned {
        float v = x[j];
        if (use_ids) {
            const unsigned w = (unsigned)j >> 5, b = 1u << (j & 31);
            if (s_seen[w] & b) v = v < 0.f ? __fmul_rn(v, pen) : __fdiv_rn(v, pen);
            if (s_ban[w] & b) v = -INFINITY;
        }
        return score_key(__fdiv_rn(v, temp));
    };
    const int chunk = (V + 255) / 256;
    const int j0 = min(V, tid * chunk), n_own = min(V, j0 + chunk) - j0;
    if (STAGED) {      // coalesced over the row; column j = t chunk + i goes to [i][t]
        for (int j = tid; j < V; j += 256) {
            const int t = j / chunk, i = j - t * chunk;
            s_stage[i * SAMPLE_STAGE_LD + t] = column_key(j);
        }
        __syncthreads();
    }
    auto own_key = [&](int i) -> unsigned { return STAGED ? s_stage[i * SAMPLE_STAGE_LD + tid] : column_key(j0 + i); };

    unsigned kmax = 0u;
#pragma unroll 4
    for (int i = 0; i < n_own; ++i) kmax = max(kmax, own_key(i));
    kmax = red.max(kmax);
    const bool empty = kmax <= KEY_NEG_INF;      // no finite score: no distribution
    const float m = key_score(kmax);
    const float u = p.u[row];
    int tok = 0, n_kept = 0;
    float logp = -INFINITY, kept_min = INFINITY;

    if (!empty && p.top_k > 0) {
        const int kk = min(p.top_k, V);
        unsigned f = 0u;
        for (int b = 31; b >= 0; --b) {
            const unsigned c = f | (1u << b);
            if (c > kmax) continue;      // (block-uniform) nothing up there
            int cnt = 0;
#pragma unroll 4
            for (int i = 0; i < n_own; ++i) cnt += own_key(i) >= c;
            const int n_ge = red.sum(cnt);
            if (n_ge >= kk) f = c;
            if (n_ge == kk) break;      // (block-uniform) key >= f is the answer; the lower bits would only move f down to the k-th key
        }
        int n_gt = 0, n_eq = 0;
        for (int i = 0; i < n_own; ++i) { const unsigned k = own_key(i); n_gt += k > f; n_eq += k == f; }
        n_gt = red.sum(n_gt);
        n_eq = red.sum(n_eq);
        const int need = kk - n_gt;      // 1 <= need <= n_eq: columns equal to f, taken by ascending column
        int col_last = V - 1;
        if (n_eq > need) {      // the largest c with count(key == f, column < c) < need: column c is the last one taken
            int c = 0;
            for (int b = 30; b >= 0; --b) {
                const int t = c | (1 << b);
                if (t >= V) continue;
                int cnt = 0;
                for (int i = 0; i < n_own; ++i) cnt += own_key(i) == f && j0 + i < t;
                if (red.sum(cnt) < need) c = t;
            }
            col_last = c;
        }
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (int i = 0; i < n_own; ++i) {
            const unsigned k = own_key(i);
            if (k > f || (k == f && j0 + i <= col_last)) {
                const int pos = atomicAdd(&s_n, 1);
                if (pos < SAMPLE_K_MAX) s_cand[pos] = ((unsigned long long)k << 32) | (unsigned)~(unsigned)(j0 + i);
            }
        }
        __syncthreads();
        if (wave == 0) {      // lane r: the candidate of rank r (keys differ, so ranks do)
            const int n = min(s_n, SAMPLE_K_MAX);
            const unsigned long long mine = lane < n ? s_cand[lane] : 0ull;
            int rank = 0;
            for (int q = 0; q < n; ++q) rank += s_cand[q] > mine;
            unsigned long long sorted = 0ull;      // lane r fetches the key whose rank is r
            for (int q = 0; q < n; ++q) {
                const unsigned long long kq = __shfl(mine, q, 64);
                const int rq = __shfl(rank, q, 64);
                if (rq == lane) sorted = kq;
            }
            const unsigned k32 = (unsigned)(sorted >> 32);
            const bool finite = lane < n && k32 > KEY_NEG_INF;
            const float s = key_score(k32);
            const float w = finite ? __expf(s - m) : 0.f;
            float incl = w;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const float o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            float excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 0.f;
            const float total = __shfl(incl, 63, 64);
            const bool kept = finite && (lane == 0 || p.top_p >= 1.f || excl < p.top_p * total);      // (a prefix of the ranks)
            const unsigned long long kept_mask = __ballot(kept);
            n_kept = __popcll(kept_mask);
            const float total_kept = __shfl(incl, n_kept - 1, 64);
            const float tgt = u * total_kept;
            const unsigned long long with_w = __ballot(kept && w > 0.f), hit = __ballot(kept && w > 0.f && incl > tgt);
            const int pick = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)with_w);      // (rank 0 always has weight 1)
            tok = (int)~(unsigned)__shfl(sorted, pick, 64);
            logp = (__shfl(s, pick, 64) - m) - logf(total_kept);
            kept_min = __shfl(s, n_kept - 1, 64);
        }
    } else if (!empty) {
        // the thread's share of mass(key > c): four interleaved partial sums, so that four reads and four chains of additions are in flight
        auto own_mass_above = [&](unsigned c) -> double {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int i = 0;
            for (; i + 4 <= n_own; i += 4) {
                const unsigned k0 = own_key(i), k1 = own_key(i + 1), k2 = own_key(i + 2), k3 = own_key(i + 3);
                a0 += k0 > c ? (double)key_weight(k0, m) : 0.0;
                a1 += k1 > c ? (double)key_weight(k1, m) : 0.0;
                a2 += k2 > c ? (double)key_weight(k2, m) : 0.0;
                a3 += k3 > c ? (double)key_weight(k3, m) : 0.0;
            }
            for (; i < n_own; ++i) { const unsigned k = own_key(i); a0 += k > c ? (double)key_weight(k, m) : 0.0; }
            return (a0 + a1) + (a2 + a3);
        };
        const double total = red.sum(own_mass_above(0u));
        double part;
        unsigned f = KEY_NEG_INF;      // kept: key > f.  top_p = 1: every finite score
        if (p.top_p < 1.f) {
            const double thr = (double)p.top_p * total;
            f = 0u;
            for (int b = 31; b >= 0; --b) {
                const unsigned c = f | (1u << b);
                if (c >= kmax) continue;      // (block-uniform) mass(key > c) = 0 < thr: the largest key is always kept
                if (red.sum(own_mass_above(c)) >= thr) f = c;
            }
            f = max(f, KEY_NEG_INF);
        }
        // the draw in column order over the kept columns (vocab_sample_kernel's walk)
        part = 0.0;
        int cnt = 0;
        unsigned kmin = 0xffffffffu;
        for (int i = 0; i < n_own; ++i) {
            const unsigned k = own_key(i);
            if (k > f) { part += (double)key_weight(k, m); ++cnt; kmin = min(kmin, k); }
        }
        double incl = part;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_scan[wave] = incl;
        n_kept = red.sum(cnt);      // (its barrier publishes s_scan)
        kmin = red.min(kmin);
        double before = 0.0;
#pragma unroll
        for (int w = 0; w < 3; ++w) before += (w < wave) ? s_scan[w] : 0.0;
        const double total_kept = ((s_scan[0] + s_scan[1]) + s_scan[2]) + s_scan[3];
        const double tgt = (double)u * total_kept;
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.0;
        double run = before + excl;
        unsigned first = 0xffffffffu, last = 0u;      // last: column + 1
        for (int i = 0; i < n_own; ++i) {
            const unsigned k = own_key(i);
            const float w = k > f ? key_weight(k, m) : 0.f;
            run += (double)w;
            if (w > 0.f) {
                last = (unsigned)(j0 + i) + 1u;
                if (run > tgt && first == 0xffffffffu) first = (unsigned)(j0 + i);
            }
        }
        first = red.min(first);
        last = red.max(last);
        tok = first != 0xffffffffu ? (int)first : (int)last - 1;      // (the largest key has weight 1: last >= 1)
        kept_min = key_score(kmin);
        if (tid == 0) logp = (key_score(column_key(tok)) - m) - (float)log(total_kept);
    }

    if (tid == 0) {
        p.token[row] = tok;
        if (p.logp) p.logp[row] = logp;
        if (p.n_kept) p.n_kept[row] = n_kept;
        if (p.kept_min) p.kept_min[row] = kept_min;
        if (appending) rid[cur_len] = tok;
        if (p.unfinished && tok == p.eos_id) {
            p.unfinished[row] = 0;
            if (p.not_done) atomicSub(p.not_done, 1);
        }
    }
}

}  // namespace

extern "C" int mico_warp_sample(const mico_warp_sample_params* p, void* stream) {
    MICO_CHECK(p, "mico_warp_sample: null parameter struct");
    MICO_CHECK(p->logits && p->u && p->token, "mico_warp_sample: null pointer");
    MICO_CHECK(p->rows >= 0 && p->V >= 1 && p->ld >= p->V, "mico_warp_sample: rows >= 0, 1 <= V <= ld (got %d, %d, %lld)", p->rows, p->V, (long long)p->ld);
    MICO_CHECK(p->top_k >= 0 && p->top_k <= SAMPLE_K_MAX, "mico_warp_sample: 0 <= top_k <= %d (got %d)", SAMPLE_K_MAX, p->top_k);
    MICO_CHECK(p->top_p > 0.f && p->top_p <= 1.f, "mico_warp_sample: top_p in (0, 1] (got %g)", (double)p->top_p);
    MICO_CHECK(p->temperature > 0.f && p->temperature <= 3.0e38f, "mico_warp_sample: temperature > 0 (got %g)", (double)p->temperature);
    if (p->ids) {
        MICO_CHECK(p->cur_len >= 0 && p->cur_len <= SAMPLE_IDS_MAX && p->ld_ids >= p->cur_len, "mico_warp_sample: 0 <= cur_len <= 512, ld_ids >= cur_len");
        MICO_CHECK(p->V <= SAMPLE_BITMAP_V, "mico_warp_sample: the processors take V <= 65536 (got %d)", p->V);
        MICO_CHECK(p->rep_penalty > 0.f && p->ngram >= 0, "mico_warp_sample: rep_penalty > 0, ngram >= 0");
        MICO_CHECK(!p->append || p->cur_len < p->ld_ids, "mico_warp_sample: append needs cur_len %d < ld_ids %lld", p->cur_len, (long long)p->ld_ids);
    }
    if (p->rows == 0) return MICO_OK;
    if (p->V <= SAMPLE_STAGE_CHUNK * 256) MICO_LAUNCH(warp_sample_kernel<true>, dim3((unsigned)p->rows), dim3(256), 0, (hipStream_t)stream, *p);
    else MICO_LAUNCH(warp_sample_kernel<false>, dim3((unsigned)p->rows), dim3(256), 0, (hipStream_t)stream, *p);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_warp_sample_params_layout(int* out, int n) {
#define OFF(F) (int)offsetof(mico_warp_sample_params, F)
    const int t[] = {(int)sizeof(mico_warp_sample_params), OFF(logits), OFF(ld), OFF(rows), OFF(V), OFF(u), OFF(ids), OFF(ld_ids), OFF(cur_len),
                     OFF(top_k), OFF(top_p), OFF(temperature), OFF(rep_penalty), OFF(ngram), OFF(ban_eos), OFF(eos_id), OFF(pad_id),
                     OFF(unfinished), OFF(not_done), OFF(append), OFF(token), OFF(logp), OFF(n_kept), OFF(kept_min), -1};
#undef OFF
    const int total = (int)(sizeof(t) / sizeof(t[0]));
    for (int i = 0; i < n && i < total; ++i) out[i] = t[i];
    return total;
}
