// Row-wise cross-entropy with label smoothing, forward and gradient in one kernel (see include/mico_hip.h).
// One 256-thread workgroup per row; online max/sum-exp in a single pass over the row (fp32 math), block reduction
// through LDS; the optional gradient pass re-reads the row (L2-resident for the small ITC/ITM rows; one extra HBM
// read for the 30522-wide LM-head rows) and writes dlogits in the GEMM's 16-bit dtype, so fp32 logits of the LM head
// never exist in HBM.
#include "common.h"

namespace {

template <typename LT> __device__ __forceinline__ float ld_logit(const LT* p, int64_t i) { return (float)p[i]; }

// LOGP (mico_logprob_fwd_bwd): row_loss receives log P(target) = x[target] - lse instead of the loss, and dscale_ptr is one upstream
// gradient PER ROW, fp32 [rows]: dlogits = dscale * dscale_ptr[row] * (onehot - softmax).  The loss instantiation is untouched by it.
template <typename LT, typename DT, bool LOGP = false>
__global__ __launch_bounds__(256) void ce_kernel(const LT* __restrict__ logits, int64_t ld, int cols,
                                                 const int64_t* __restrict__ target, int ignore_index, float ls,
                                                 float lscale, float* __restrict__ row_loss, float* __restrict__ row_lse,
                                                 DT* __restrict__ dlogits, int64_t ld_d, const float* __restrict__ dscale_ptr,
                                                 float dscale) {
    __shared__ float red[3][4];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LT* x = logits + row * ld;
    const int64_t t = target[row];
    const bool ignored = (t == ignore_index) || t < 0 || t >= cols;
    float m = -1.0e30f, s = 0.f, sx = 0.f;
    for (int c = tid; c < cols; c += 256) {
        const float v = ld_logit(x, c) * lscale;
        sx += v;
        if (v > m) { s = s * __expf(m - v) + 1.f; m = v; }
        else s += __expf(v - m);
    }
    // wave reduce (m, s), then block
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const float mn = fmaxf(m, m2);
        s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
        m = mn;
        sx += __shfl_xor(sx, o, 64);
    }
    if (lane == 0) { red[0][wave] = m; red[1][wave] = s; red[2][wave] = sx; }
    __syncthreads();
    float M = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    float S = 0.f, SX = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) { S += red[1][w] * __expf(red[0][w] - M); SX += red[2][w]; }
    const float lse = M + __logf(S);
    if (tid == 0) {
        float loss = 0.f;
        if (!ignored) {
            const float xt = ld_logit(x, t) * lscale;
            if constexpr (LOGP) loss = xt - lse;
            else loss = (1.f - ls) * (lse - xt) + ls * (lse - SX / (float)cols);
        }
        if (row_loss) row_loss[row] = loss;
        if (row_lse) row_lse[row] = lse;
    }
    if (!dlogits) return;
    float ds = dscale * lscale;
    if constexpr (LOGP) ds *= -dscale_ptr[row];      // (softmax - onehot) below, the other sign
    else if (dscale_ptr) ds *= dscale_ptr[0];
    if (ignored) ds = 0.f;
    const float smooth = ls / (float)cols;
    DT* d = dlogits + row * ld_d;
    for (int c = tid; c < cols; c += 256) {
        const float v = ld_logit(x, c) * lscale;
        float gsm = __expf(v - lse) - smooth;
        if (c == t) gsm -= (1.f - ls);
        d[c] = (DT)(gsm * ds);
    }
}

// ITM hard-negative draw (vast.py:423-440): one wave per row, every lane a contiguous chunk of the row (the row is read three times
// from L1: max, sum of exponentials, weights).  idx = #{j : cdf_j < u * total} is a pure counting problem once every lane knows the
// exclusive prefix of its chunk, so no lane has to be singled out.
__global__ __launch_bounds__(64) void itm_sample_kernel(const float* __restrict__ sim, int64_t ld, int cols, int diag_offset,
                                                        const float* __restrict__ u, int64_t* __restrict__ out) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* x = sim + (int64_t)row * ld;
    const int chunk = (cols + 63) / 64;
    const int j0 = min(cols, lane * chunk), j1 = min(cols, j0 + chunk);
    float m = -3.0e38f;
    for (int j = j0; j < j1; ++j) m = fmaxf(m, x[j]);
    m = wave_max(m);
    float se = 0.f;
    for (int j = j0; j < j1; ++j) se += __expf(x[j] - m);
    se = wave_sum(se);
    const float inv = 1.f / se;
    const int dcol = diag_offset + row;
    float part = 0.f;
    for (int j = j0; j < j1; ++j) part += (j == dcol) ? 0.f : fmaf(__expf(x[j] - m), inv, 1e-4f);
    float incl = part;   // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    const float total = __shfl(incl, 63, 64);
    const float tgt = u[row] * total;
    float run = incl - part;
    int cnt = 0;
    for (int j = j0; j < j1; ++j) {
        run += (j == dcol) ? 0.f : fmaf(__expf(x[j] - m), inv, 1e-4f);
        cnt += run <= tgt;     // first column whose CDF exceeds the target: a zero-weight column (the diagonal) is never chosen
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if (lane == 0) {
        if (cnt >= cols) cnt = (dcol == cols - 1) ? cols - 2 : cols - 1;   // u * total rounded up to the total: the last column with weight
        out[row] = max(cnt, 0);
    }
}

// Full-vocabulary draw (mico_vocab_sample): one 256-thread workgroup per row, every thread a contiguous chunk of the row, which is read
// three times (max; weights e^(x - max) summed per chunk; the search) - the second and third time from L2.  The running sum of column j is
// (exclusive block scan of the chunk sums) + (the chunk's own sequential sum up to j), `total` the scan's last value.  The drawn column is
// found as a minimum over the columns that qualify (running sum above u * total AND a non-zero weight), so a zero-weight column cannot be
// drawn whatever the rounding at a chunk boundary does; when no column qualifies (u * total rounded up to the total) it is the last
// column with a weight.
__global__ __launch_bounds__(256) void vocab_sample_kernel(const float* __restrict__ logits, int64_t ld, int cols, const float* __restrict__ u,
                                                           unsigned char* __restrict__ unfinished, int eos, int pad,
                                                           int64_t* __restrict__ token, float* __restrict__ logp) {
    __shared__ float redf[4];
    __shared__ int redi[2][4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (unfinished && !unfinished[row]) {       // (block-uniform)
        if (tid == 0) { token[row] = pad; logp[row] = 0.f; }
        return;
    }
    const float* x = logits + (int64_t)row * ld;
    const int chunk = (cols + 255) / 256;
    const int j0 = min(cols, tid * chunk), j1 = min(cols, j0 + chunk);
    float m = -3.0e38f;
    for (int j = j0; j < j1; ++j) m = fmaxf(m, x[j]);
    m = wave_max(m);
    if (lane == 0) redf[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    __syncthreads();
    float part = 0.f;
    for (int j = j0; j < j1; ++j) part += __expf(x[j] - m);
    float incl = part;      // inclusive scan over the lanes, then over the waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) redf[wave] = incl;
    __syncthreads();
    float before = 0.f;
#pragma unroll
    for (int w = 0; w < 3; ++w) before += (w < wave) ? redf[w] : 0.f;
    const float total = ((redf[0] + redf[1]) + redf[2]) + redf[3];
    const float tgt = u[row] * total;
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    float run = before + excl;
    int first = cols, last = -1;
    for (int j = j0; j < j1; ++j) {
        const float w = __expf(x[j] - m);
        run += w;
        if (w > 0.f) {
            last = j;
            if (run > tgt && first == cols) first = j;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        first = min(first, __shfl_xor(first, d, 64));
        last = max(last, __shfl_xor(last, d, 64));
    }
    if (lane == 0) { redi[0][wave] = first; redi[1][wave] = last; }
    __syncthreads();
    if (tid == 0) {
        first = min(min(redi[0][0], redi[0][1]), min(redi[0][2], redi[0][3]));
        last = max(max(redi[1][0], redi[1][1]), max(redi[1][2], redi[1][3]));
        const int tok = first < cols ? first : max(last, 0);      // (no column with a weight at all - nothing finite in the row: column 0)
        token[row] = tok;
        logp[row] = last < 0 ? -INFINITY : x[tok] - (m + logf(total));
        if (unfinished && tok == eos) unfinished[row] = 0;
    }
}

// Row-wise top-k (mico_topk_rows): one wave per row, ONE pass over the row.  Every element becomes a 64-bit key - the value's bits made
// monotonic in the high word, ~column in the low word - so the order is total: larger value first, equal values by ascending column, NaN last.
// The wave keeps the best TOPK_MAX keys seen so far sorted in LDS next to a staging area of the same size; an element enters the staging area only
// if its key beats the current k-th best (for a random row that happens ~k ln(cols / k) times in all), and a full staging area is folded in by a
// 256-key bitonic sort.  A row sorted ascending is the worst case: a sort per 65 .. 128 elements.
constexpr int TOPK_MAX = 128;

__device__ __forceinline__ unsigned long long topk_key(float v, int col) {
    v += 0.f;                                           // -0 -> +0: equal values tie-break by column
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // monotonic in the value
    if (v != v) u = 0u;                                 // NaN below -inf
    return ((unsigned long long)u << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)col);
}

__device__ __forceinline__ void topk_sort256(unsigned long long* buf, int lane) {   // descending; one wave; 36 compare-exchange steps, fully
#pragma unroll                                                                      // unrolled: every stride and direction mask is a constant
    for (int size = 2; size <= 2 * TOPK_MAX; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int t = lane + r * 64;
                const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
                const unsigned long long a = buf[lo], b = buf[hi];
                const bool desc = (lo & size) == 0;
                if (desc ? a < b : a > b) { buf[lo] = b; buf[hi] = a; }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void topk_rows_kernel(const float* __restrict__ sim, int64_t ld, int cols, int k, int* __restrict__ idx_out,
                                                       float* __restrict__ val_out) {
    __shared__ unsigned long long buf[2 * TOPK_MAX];    // [0, TOPK_MAX): best so far, sorted; [TOPK_MAX, 2 TOPK_MAX): staging
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* x = sim + (int64_t)row * ld;
    for (int i = lane; i < 2 * TOPK_MAX; i += 64) buf[i] = 0ull;   // 0 is below every real key
    __syncthreads();
    unsigned long long thr = 0ull;
    int cnt = 0;                                        // staged keys (wave-uniform)
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    float cur[4], nxt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int c = j * 64 + lane; cur[j] = c < cols ? x[c] : 0.f; }
    for (int c0 = 0; c0 < cols; c0 += 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int c = c0 + 256 + j * 64 + lane; nxt[j] = c < cols ? x[c] : 0.f; }   // next block in flight
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * 64 + lane;
            if (c0 + j * 64 >= cols) break;             // (wave-uniform)
            if (cnt > TOPK_MAX - 64) {                  // the next 64 elements might not fit: fold the staging area in
                for (int i = cnt + lane; i < TOPK_MAX; i += 64) buf[TOPK_MAX + i] = 0ull;
                __syncthreads();
                topk_sort256(buf, lane);
                thr = buf[k - 1];
                cnt = 0;
                __syncthreads();
            }
            const unsigned long long key = topk_key(cur[j], c);
            const bool pass = c < cols && key > thr;
            const unsigned long long m = __ballot(pass);
            if (pass) buf[TOPK_MAX + cnt + __popcll(m & lt_mask)] = key;
            cnt += __popcll(m);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    if (cnt > 0) {
        for (int i = cnt + lane; i < TOPK_MAX; i += 64) buf[TOPK_MAX + i] = 0ull;
        __syncthreads();
        topk_sort256(buf, lane);
    }
    __syncthreads();
    for (int i = lane; i < k; i += 64) {
        const unsigned long long key = buf[i];
        const unsigned o = (unsigned)(key >> 32);
        idx_out[(int64_t)row * k + i] = (int)(0xFFFFFFFFu - (unsigned)key);
        if (val_out) val_out[(int64_t)row * k + i] = __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
    }
}

}  // namespace

// TokenMasker.perform_mask (data/model/general_module.py:64-97) with the random numbers supplied by the caller: one wave per row.
__global__ __launch_bounds__(64) void token_mask_kernel(const int64_t* __restrict__ tokens, int S, float mask_prob, const float* __restrict__ u_mask,
                                                        int rounds, int64_t round_stride, const float* __restrict__ u_kind,
                                                        const float* __restrict__ u_tok, int mask_token, int range_start, int range_end,
                                                        int64_t* __restrict__ out_tokens, int64_t* __restrict__ labels) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int64_t* t = tokens + (int64_t)row * S;
    // indicator: position 0 and pads (id 0) are never masked; a row is re-drawn (next round of uniforms) until it has >= 1 masked token
    unsigned long long any = 0;
    int r = 0;
    for (; r < rounds && !any; ++r) {
        const float* u = u_mask + r * round_stride + (int64_t)row * S;
        for (int j0 = 0; j0 < S; j0 += 64) {
            const int j = j0 + lane;
            const bool hit = j >= 1 && j < S && t[j] != 0 && u[j] < mask_prob;
            any |= __ballot(hit);
        }
    }
    const int used = r - 1;   // the round whose draw stands
    // `rounds` exhausted with nothing selected: the reference would keep drawing (general_module.py:71 guarantees >= 1 masked token per
    // row), so ONE maskable position is forced - the floor(u_tok[row][0] * n)-th of the row's n maskable positions (u_tok of position 0 is
    // otherwise unused: position 0 is never masked).  A row without any maskable token keeps nothing masked.
    int forced = -1;
    if (!any) {
        int n = 0;
        for (int j0 = 0; j0 < S; j0 += 64) {
            const int j = j0 + lane;
            n += __popcll(__ballot(j >= 1 && j < S && t[j] != 0));
        }
        if (n > 0) {
            int k = (int)(u_tok[(int64_t)row * S] * (float)n);
            k = k < n ? k : n - 1;
            for (int j0 = 0; j0 < S && forced < 0; j0 += 64) {
                const int j = j0 + lane;
                unsigned long long m = __ballot(j >= 1 && j < S && t[j] != 0);
                const int c = __popcll(m);
                if (k < c) {
                    for (int q = 0; q < k; ++q) m &= m - 1;     // drop the k lowest set bits
                    forced = j0 + __ffsll((long long)m) - 1;
                } else k -= c;
            }
        }
    }
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        if (j >= S) break;
        const int64_t src = t[j];
        const bool hit = any ? (j >= 1 && src != 0 && u_mask[used * round_stride + (int64_t)row * S + j] < mask_prob) : j == forced;
        int64_t tok = src, lab = -100;
        if (hit) {
            lab = src;
            const float pk = u_kind[(int64_t)row * S + j];
            if (pk < 0.8f) tok = mask_token;
            else if (pk < 0.9f) {
                int c = range_start + (int)(u_tok[(int64_t)row * S + j] * (float)(range_end - range_start));
                tok = c < range_end ? c : range_end - 1;
            }
        }
        out_tokens[(int64_t)row * S + j] = tok;
        labels[(int64_t)row * S + j] = lab;
    }
}

extern "C" int mico_token_mask(const int64_t* tokens, int rows, int S, float mask_prob, const float* u_mask, int rounds, const float* u_kind,
                               const float* u_tok, int mask_token, int range_start, int range_end, int64_t* out_tokens, int64_t* labels,
                               void* stream) {
    MICO_CHECK(tokens && u_mask && u_kind && u_tok && out_tokens && labels && rows > 0 && S > 0 && rounds > 0, "mico_token_mask: bad args");
    MICO_CHECK(range_end > range_start && mask_prob >= 0.f && mask_prob <= 1.f, "mico_token_mask: bad range / probability");
    MICO_LAUNCH(token_mask_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, tokens, S, mask_prob, u_mask, rounds, (int64_t)rows * S, u_kind, u_tok,
                mask_token, range_start, range_end, out_tokens, labels);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_itm_sample(const float* sim, int64_t ld, int rows, int cols, int diag_offset, const float* u, int64_t* out,
                               void* stream) {
    MICO_CHECK(sim && u && out && cols > 0 && ld >= cols, "mico_itm_sample: bad args");
    if (rows <= 0) return MICO_OK;
    MICO_LAUNCH(itm_sample_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, sim, ld, cols, diag_offset, u, out);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_topk_rows(const float* sim, int64_t row_stride, int rows, int cols, int k, int* idx_out, float* val_out, void* stream) {
    MICO_CHECK(sim && idx_out && cols > 0 && row_stride >= cols, "mico_topk_rows: bad args");
    MICO_CHECK(k >= 1 && k <= TOPK_MAX && k <= cols, "mico_topk_rows: k must be in [1, %d] and <= cols (got k = %d, cols = %d)", TOPK_MAX, k, cols);
    if (rows <= 0) return MICO_OK;
    MICO_LAUNCH(topk_rows_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, sim, row_stride, cols, k, idx_out, val_out);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_ce_fwd_bwd(const void* logits, int logits_dtype, int64_t ld, int64_t rows, int cols,
                               const int64_t* target, int ignore_index, float label_smoothing, float logits_scale,
                               float* row_loss, float* row_lse, void* dlogits, int dlogits_dtype, int64_t ld_d,
                               const float* dscale_ptr, float dscale, int dtype, void* stream) {
    MICO_CHECK(logits && target && cols > 0, "mico_ce_fwd_bwd: bad args");
    MICO_CHECK(logits_dtype == MICO_F32 || logits_dtype == MICO_F16 || logits_dtype == MICO_BF16, "mico_ce_fwd_bwd: logits dtype");
    MICO_CHECK(!dlogits || dlogits_dtype == logits_dtype, "mico_ce_fwd_bwd: dlogits dtype must equal the logits dtype");
    (void)dtype;
    if (rows <= 0) return MICO_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)rows), block(256);
#define CE(LT) MICO_LAUNCH((ce_kernel<LT, LT>), grid, block, 0, st, (const LT*)logits, ld, cols, target, ignore_index, label_smoothing, logits_scale, row_loss, row_lse, (LT*)dlogits, ld_d, dscale_ptr, dscale)
    if (logits_dtype == MICO_F32) CE(float);
    else if (logits_dtype == MICO_F16) CE(f16);
    else CE(bf16);
#undef CE
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_logprob_fwd_bwd(const void* logits, int logits_dtype, int64_t ld, int64_t rows, int cols, const int64_t* target,
                                    int ignore_index, float* row_logp, void* dlogits, int64_t ld_d, const float* row_gscale, float gscale,
                                    void* stream) {
    MICO_CHECK(logits && target && cols > 0 && ld >= cols, "mico_logprob_fwd_bwd: bad args");
    MICO_CHECK(logits_dtype == MICO_F32 || logits_dtype == MICO_F16 || logits_dtype == MICO_BF16, "mico_logprob_fwd_bwd: logits dtype");
    MICO_CHECK(!dlogits || (row_gscale && ld_d >= cols), "mico_logprob_fwd_bwd: the gradient pass needs row_gscale [rows] and ld_d >= cols");
    if (rows <= 0) return MICO_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)rows), block(256);
#define LP(LT) MICO_LAUNCH((ce_kernel<LT, LT, true>), grid, block, 0, st, (const LT*)logits, ld, cols, target, ignore_index, 0.f, 1.f, row_logp, (float*)nullptr, (LT*)dlogits, ld_d, row_gscale, gscale)
    if (logits_dtype == MICO_F32) LP(float);
    else if (logits_dtype == MICO_F16) LP(f16);
    else LP(bf16);
#undef LP
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_vocab_sample(const float* logits, int64_t ld, int rows, int cols, const float* u, unsigned char* unfinished, int eos_id,
                                 int pad_id, int64_t* token, float* logp, void* stream) {
    MICO_CHECK(logits && u && token && logp && cols > 0 && ld >= cols, "mico_vocab_sample: bad args");
    if (rows <= 0) return MICO_OK;
    MICO_LAUNCH(vocab_sample_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, ld, cols, u, unfinished, eos_id, pad_id, token,
                logp);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}
