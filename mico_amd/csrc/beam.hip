// Beam search on the device (include/mico_hip.h, "Device-side beam search"): the per-step candidate selection with the logits processors
// (mico_beam_topk) and the bookkeeping of transformers' BeamSearchScorer / BeamHypotheses (mico_beam_step, mico_beam_finalize).
#include "common.h"
#include <stddef.h>

namespace {

constexpr int BEAM_NB_MAX = 8;
constexpr int BEAM_K_MAX = 2 * BEAM_NB_MAX;      // candidates per set and step
constexpr int BEAM_BITMAP_V = 65536;             // largest vocabulary of the processors' two bitmaps
constexpr int BEAM_IDS_MAX = 512;

// A candidate as one 64-bit key: the score's bits made monotonic in the high word, ~(beam * V + token) in the low word - larger score first,
// equal scores by ascending flat index, NaN last (topk_rows_kernel's order).  Keys of different candidates differ.
__device__ __forceinline__ unsigned long long beam_key(float v, unsigned flat) {
    v += 0.f;                                           // -0 -> +0
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (v != v) u = 0u;
    return ((unsigned long long)u << 32) | (unsigned)~flat;
}
__device__ __forceinline__ float beam_key_score(unsigned long long k) {
    const unsigned u = (unsigned)(k >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(k, d, 64);
        k = o > k ? o : k;
    }
    return k;
}

// One 256-thread workgroup per row.  Pass 1: online log-sum-exp over the row (column j = tid + 256 i: coalesced).  Pass 2 (the row comes from
// L2): every column's processed score + beam score becomes a key; a thread keeps the K = 2 nb best of its own columns sorted in its LDS column
// s_list[.][tid] (an insertion happens only when a key beats the thread's K-th best: ~K ln(n / K) times for n random columns).  The 256 lists
// are merged by K rounds of "largest head".  The processors are two bitmaps over the vocabulary (seen, banned), built from the row's ids.
__global__ __launch_bounds__(256) void beam_row_kernel(const float* __restrict__ logits, int64_t ld, int nb, int V, const float* __restrict__ beam_scores,
                                                       const unsigned char* __restrict__ done, const int64_t* __restrict__ ids, int64_t ld_ids,
                                                       int cur_len, float pen, int ngram, int ban_eos, int eos, unsigned long long* __restrict__ ws) {
    __shared__ unsigned long long s_list[BEAM_K_MAX][256];
    __shared__ unsigned s_seen[BEAM_BITMAP_V / 32], s_ban[BEAM_BITMAP_V / 32];
    __shared__ float s_m[4], s_s[4];
    __shared__ unsigned long long s_red[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int set = row / nb, beam = row - set * nb, K = 2 * nb;
    if (done && done[set]) return;      // (block-uniform)
    const float* x = logits + (int64_t)row * ld;

    float m = -3.0e38f, s = 0.f;
    for (int j = tid; j < V; j += 256) {
        const float v = x[j], mn = fmaxf(m, v);
        s = s * __expf(m - mn) + __expf(v - mn);
        m = mn;
    }
    const float wm = wave_max(m);
    s = wave_sum(s * __expf(m - wm));
    if (lane == 0) { s_m[wave] = wm; s_s[wave] = s; }
    const bool use_ids = ids != nullptr;
    if (use_ids)
        for (int i = tid; i < (V + 31) / 32; i += 256) { s_seen[i] = 0u; s_ban[i] = 0u; }
#pragma unroll
    for (int k = 0; k < BEAM_K_MAX; ++k)
        if (k < K) s_list[k][tid] = 0ull;
    __syncthreads();
    const float M = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) S += s_s[w] * __expf(s_m[w] - M);
    const float log_s = logf(S);      // score = (x - max) - log(sum), the order torch's log_softmax takes

    if (use_ids) {
        const int64_t* rid = ids + (int64_t)row * ld_ids;
        if (pen != 1.f)
            for (int i = tid; i < cur_len; i += 256) {
                const int64_t t = rid[i];
                if (t >= 0 && t < V) atomicOr(&s_seen[t >> 5], 1u << (t & 31));
            }
        if (ngram > 0 && cur_len >= ngram) {
            const int nwin = cur_len - ngram + 1, tail = cur_len - ngram + 1;      // windows [i, i + ngram); the last ngram - 1 ids start at `tail`
            for (int i = tid; i < nwin; i += 256) {
                bool match = true;
                for (int q = 0; q < ngram - 1; ++q) match = match && rid[i + q] == rid[tail + q];
                const int64_t t = rid[i + ngram - 1];
                if (match && t >= 0 && t < V) atomicOr(&s_ban[t >> 5], 1u << (t & 31));
            }
        }
        if (ban_eos && tid == 0 && eos >= 0 && eos < V) atomicOr(&s_ban[eos >> 5], 1u << (eos & 31));
        __syncthreads();
    }

    const float bs = beam_scores[row];
    const unsigned flat0 = (unsigned)beam * (unsigned)V;
    unsigned long long kth = 0ull;      // the thread's K-th best so far
    for (int j = tid; j < V; j += 256) {
        float v = __fsub_rn(__fsub_rn(x[j], M), log_s);
        if (use_ids) {
            const unsigned w = (unsigned)j >> 5, b = 1u << (j & 31);
            if (s_seen[w] & b) v = v < 0.f ? __fmul_rn(v, pen) : __fdiv_rn(v, pen);
            if (s_ban[w] & b) v = -INFINITY;
        }
        const unsigned long long key = beam_key(__fadd_rn(v, bs), flat0 + (unsigned)j);
        if (key > kth) {
            int i = K - 1;
            while (i > 0 && s_list[i - 1][tid] < key) {
                s_list[i][tid] = s_list[i - 1][tid];
                --i;
            }
            s_list[i][tid] = key;
            kth = s_list[K - 1][tid];
        }
    }

    int head = 0;
    for (int r = 0; r < K; ++r) {
        const unsigned long long mine = head < K ? s_list[head][tid] : 0ull;
        const unsigned long long wbest = wave_max_u64(mine);
        if (lane == 0) s_red[wave] = wbest;
        __syncthreads();
        unsigned long long best = s_red[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) best = s_red[w] > best ? s_red[w] : best;
        if (best != 0ull && mine == best) ++head;
        if (tid == 0) ws[(int64_t)row * K + r] = best;
        __syncthreads();
    }
}

// One wave per set: the nb rows' K-lists (nb K <= 128 keys) are ranked by counting; ranks below K are the set's candidates.
__global__ __launch_bounds__(64) void beam_set_kernel(const unsigned long long* __restrict__ ws, int nb, int V, const unsigned char* __restrict__ done,
                                                      float* __restrict__ out_score, int* __restrict__ out_beam, int* __restrict__ out_token) {
    __shared__ unsigned long long s_k[BEAM_NB_MAX * BEAM_K_MAX];
    const int set = blockIdx.x, lane = threadIdx.x, K = 2 * nb, n = nb * K;
    if (done && done[set]) return;
    for (int i = lane; i < n; i += 64) s_k[i] = ws[(int64_t)set * n + i];
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const unsigned long long k = s_k[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (s_k[j] > k) || (s_k[j] == k && j < i);
        if (rank < K) {
            const unsigned flat = ~(unsigned)k;
            const unsigned b = flat / (unsigned)V;
            out_score[(int64_t)set * K + rank] = beam_key_score(k);
            out_beam[(int64_t)set * K + rank] = (int)(b < (unsigned)nb ? b : (unsigned)nb - 1u);
            out_token[(int64_t)set * K + rank] = (int)(flat - b * (unsigned)V);
        }
    }
}

// ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
// The n-best list of one set (BeamHypotheses), held by every lane of the set's wave in registers: the same values in all 64 lanes, every
// branch wave-uniform, loops unrolled over the 8 slots so that no array is indexed at run time.  Slots are in insertion order.
struct BeamList {
    double score[BEAM_NB_MAX];
    int len[BEAM_NB_MAX];
    int count;
    double worst;
};

__device__ __forceinline__ void beam_list_load(const mico_beam_params& p, int set, BeamList& st) {
    st.count = min(max(p.hyp_count[set], 0), p.nb);
    st.worst = p.worst[set];
#pragma unroll
    for (int k = 0; k < BEAM_NB_MAX; ++k) {
        st.score[k] = k < p.nb ? p.hyp_score[set * p.nb + k] : 0.0;
        st.len[k] = k < p.nb ? p.hyp_len[set * p.nb + k] : 0;
    }
}
__device__ __forceinline__ void beam_list_store(const mico_beam_params& p, int set, const BeamList& st, int lane) {
    if (lane != 0) return;
    p.hyp_count[set] = st.count;
    p.worst[set] = st.worst;
#pragma unroll
    for (int k = 0; k < BEAM_NB_MAX; ++k)
        if (k < p.nb) {
            p.hyp_score[set * p.nb + k] = st.score[k];
            p.hyp_len[set * p.nb + k] = st.len[k];
        }
}
__device__ __forceinline__ void beam_copy_ids(int64_t* dst, const int64_t* src, int n, int lane) {
    for (int i = lane; i < n; i += 64) dst[i] = src[i];
}

// BeamHypotheses.add(src[:len], sum_logprob): score = sum_logprob / len ** length_penalty in fp64 against the caller's table; a full list takes
// the hypothesis only if it beats `worst`, drops its lowest entry (the earliest of equals) and closes the gap, so the order stays insertion order.
__device__ void beam_list_add(const mico_beam_params& p, int set, BeamList& st, const int64_t* src, int len, float sum_logprob, int lane) {
    const int nb = p.nb;
    const double score = (double)sum_logprob / p.len_pow[len];
    if (!(st.count < nb || score > st.worst)) return;
    int64_t* H = p.hyp_ids + (int64_t)set * nb * p.max_length;
    const bool evict = st.count == nb;
    if (evict) {
        int lo = 0;
        double lo_s = st.score[0];
#pragma unroll
        for (int k = 1; k < BEAM_NB_MAX; ++k)
            if (k < nb && st.score[k] < lo_s) { lo = k; lo_s = st.score[k]; }
#pragma unroll
        for (int k = 0; k < BEAM_NB_MAX - 1; ++k)
            if (k >= lo && k < nb - 1) {      // (a lane re-reads only positions it wrote itself)
                beam_copy_ids(H + (int64_t)k * p.max_length, H + (int64_t)(k + 1) * p.max_length, st.len[k + 1], lane);
                st.score[k] = st.score[k + 1];
                st.len[k] = st.len[k + 1];
            }
        st.count = nb - 1;
    }
    const int slot = st.count;
    beam_copy_ids(H + (int64_t)slot * p.max_length, src, len, lane);
    double w = score;
#pragma unroll
    for (int k = 0; k < BEAM_NB_MAX; ++k) {
        if (k == slot) { st.score[k] = score; st.len[k] = len; }
        if (k < slot) w = fmin(w, st.score[k]);
    }
    st.count = slot + 1;
    st.worst = evict ? w : fmin(score, st.worst);      // after an eviction: the lowest of what stayed
}

// row r of the next step: score, parent row, ids_out[r] = ids_in[parent, :cur_len] + token
__device__ __forceinline__ void beam_emit(const mico_beam_params& p, int r, float score, int parent, int token, int lane) {
    beam_copy_ids(p.ids_out + (int64_t)r * p.max_length, p.ids_in + (int64_t)parent * p.max_length, p.cur_len, lane);
    if (lane == 0) {
        p.beam_scores[r] = score;
        p.parent[r] = parent;
        p.ids_out[(int64_t)r * p.max_length + p.cur_len] = token;
    }
}

__global__ __launch_bounds__(64) void beam_step_kernel(const mico_beam_params p) {
    const int set = blockIdx.x, lane = threadIdx.x, nb = p.nb, K = 2 * nb;
    int k = 0;
    if (!p.done[set]) {
        BeamList st;
        beam_list_load(p, set, st);
        for (int rank = 0; rank < K && k < nb; ++rank) {
            const float s = p.cand_score[set * K + rank];
            const int b = min(max(p.cand_beam[set * K + rank], 0), nb - 1), t = p.cand_token[set * K + rank];
            const int row = set * nb + b;
            if (p.eos_id >= 0 && t == p.eos_id) {
                if (rank < nb) beam_list_add(p, set, st, p.ids_in + (int64_t)row * p.max_length, p.cur_len, s, lane);
            } else {
                beam_emit(p, set * nb + k, s, row, t, lane);
                ++k;
            }
        }
        beam_list_store(p, set, st, lane);
        // BeamHypotheses.is_done(best candidate, cur_len + 1)
        if (st.count >= nb && st.worst >= (double)p.cand_score[set * K] / p.len_pow[p.cur_len + 1] && lane == 0) {
            p.done[set] = 1;
            atomicSub(p.not_done, 1);
        }
    }
    for (; k < nb; ++k) beam_emit(p, set * nb + k, 0.f, set * nb + k, p.pad_id, lane);      // a done set: pad, its own rows as parents
}

__global__ __launch_bounds__(64) void beam_finalize_kernel(const mico_beam_params p) {
    const int set = blockIdx.x, lane = threadIdx.x, nb = p.nb;
    BeamList st;
    beam_list_load(p, set, st);
    if (!p.done[set]) {
        for (int k = 0; k < nb; ++k)
            beam_list_add(p, set, st, p.ids_in + (int64_t)(set * nb + k) * p.max_length, p.cur_len, p.beam_scores[set * nb + k], lane);
        beam_list_store(p, set, st, lane);
        if (lane == 0) {
            p.done[set] = 1;
            atomicSub(p.not_done, 1);
        }
    }
    int best = 0, len = st.count > 0 ? st.len[0] : 0;
    double best_s = st.score[0];
#pragma unroll
    for (int k = 1; k < BEAM_NB_MAX; ++k)
        if (k < st.count && st.score[k] > best_s) { best = k; best_s = st.score[k]; len = st.len[k]; }
    len = min(max(len, 0), p.max_length);
    const int64_t* h = p.hyp_ids + ((int64_t)set * nb + best) * p.max_length;
    int64_t* out = p.best_ids + (int64_t)set * p.max_length;
    for (int i = lane; i < p.max_length; i += 64) out[i] = i < len ? h[i] : (i == len && p.eos_id >= 0 ? p.eos_id : p.pad_id);
    if (lane == 0) p.best_len[set] = len;
}

int beam_params_check(const mico_beam_params* p, const char* who, bool finalize) {
    MICO_CHECK(p, "%s: null parameter struct", who);
    MICO_CHECK(p->sets >= 0 && p->nb >= 1 && p->nb <= BEAM_NB_MAX, "%s: sets >= 0, 1 <= nb <= 8", who);
    MICO_CHECK(p->max_length >= 1 && p->cur_len >= 0 && p->cur_len + (finalize ? 0 : 1) <= p->max_length,
               "%s: cur_len %d does not fit max_length %d", who, p->cur_len, p->max_length);
    MICO_CHECK(p->len_pow && p->ids_in && p->beam_scores && p->hyp_ids && p->hyp_len && p->hyp_score && p->hyp_count && p->worst && p->done &&
               p->not_done, "%s: null pointer", who);
    if (finalize) MICO_CHECK(p->best_ids && p->best_len, "%s: null pointer", who);
    else MICO_CHECK(p->cand_score && p->cand_beam && p->cand_token && p->ids_out && p->parent && p->ids_out != p->ids_in, "%s: null pointer, or ids_out is ids_in", who);
    MICO_CHECK((int64_t)p->sets * p->nb <= 0x7fffffff / 2 / BEAM_NB_MAX, "%s: too many rows", who);
    return MICO_OK;
}

}  // namespace

extern "C" int mico_beam_topk(const float* logits, int64_t ld, int sets, int nb, int V, const float* beam_scores, const unsigned char* done,
                              const int64_t* ids, int64_t ld_ids, int cur_len, float rep_penalty, int ngram, int ban_eos, int eos_id,
                              void* ws, float* out_score, int* out_beam, int* out_token, void* stream) {
    MICO_CHECK(logits && beam_scores && ws && out_score && out_beam && out_token, "mico_beam_topk: null pointer");
    MICO_CHECK(sets >= 0 && nb >= 1 && nb <= BEAM_NB_MAX, "mico_beam_topk: sets >= 0, 1 <= nb <= 8 (got %d, %d)", sets, nb);
    MICO_CHECK(V >= 2 * nb && ld >= V && (int64_t)nb * V <= 0x7fffffff, "mico_beam_topk: 2 nb <= V <= ld, nb V < 2^31");
    MICO_CHECK((int64_t)sets * nb <= 0x7fffffff / BEAM_K_MAX, "mico_beam_topk: too many rows");
    MICO_CHECK((((uintptr_t)ws) & 7) == 0, "mico_beam_topk: ws must be 8-byte aligned");
    if (ids) {
        MICO_CHECK(cur_len >= 0 && cur_len <= BEAM_IDS_MAX && ld_ids >= cur_len, "mico_beam_topk: 0 <= cur_len <= 512, ld_ids >= cur_len");
        MICO_CHECK(V <= BEAM_BITMAP_V, "mico_beam_topk: the processors take V <= 65536 (got %d)", V);
        MICO_CHECK(rep_penalty > 0.f && ngram >= 0, "mico_beam_topk: rep_penalty > 0, ngram >= 0");
    }
    if (sets == 0) return MICO_OK;
    MICO_LAUNCH(beam_row_kernel, dim3((unsigned)(sets * nb)), dim3(256), 0, (hipStream_t)stream, logits, ld, nb, V, beam_scores, done, ids, ld_ids,
                cur_len, rep_penalty, ngram, ban_eos, eos_id, (unsigned long long*)ws);
    MICO_LAUNCH_CHECK();
    MICO_LAUNCH(beam_set_kernel, dim3((unsigned)sets), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)ws, nb, V, done, out_score,
                out_beam, out_token);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_beam_step(const mico_beam_params* p, void* stream) {
    if (int rc = beam_params_check(p, "mico_beam_step", false)) return rc;
    if (p->sets == 0) return MICO_OK;
    MICO_LAUNCH(beam_step_kernel, dim3((unsigned)p->sets), dim3(64), 0, (hipStream_t)stream, *p);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_beam_finalize(const mico_beam_params* p, void* stream) {
    if (int rc = beam_params_check(p, "mico_beam_finalize", true)) return rc;
    if (p->sets == 0) return MICO_OK;
    MICO_LAUNCH(beam_finalize_kernel, dim3((unsigned)p->sets), dim3(64), 0, (hipStream_t)stream, *p);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_beam_params_layout(int* out, int n) {
#define OFF(F) (int)offsetof(mico_beam_params, F)
    const int t[] = {(int)sizeof(mico_beam_params), OFF(sets), OFF(nb), OFF(cur_len), OFF(max_length), OFF(eos_id), OFF(pad_id), OFF(cand_score),
                     OFF(cand_beam), OFF(cand_token), OFF(len_pow), OFF(ids_in), OFF(ids_out), OFF(beam_scores), OFF(parent), OFF(hyp_ids),
                     OFF(hyp_len), OFF(hyp_score), OFF(hyp_count), OFF(worst), OFF(done), OFF(not_done), OFF(best_ids), OFF(best_len), -1};
#undef OFF
    const int total = (int)(sizeof(t) / sizeof(t[0]));
    for (int i = 0; i < n && i < total; ++i) out[i] = t[i];
    return total;
}
