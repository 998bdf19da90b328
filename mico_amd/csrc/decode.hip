// Incremental caption decoding (functional.BertDecodeCache): grouped-query decode attention over a key split, and the two
// K/V-cache upkeep launches (append of a pass's new positions, beam re-gather by parent row).  Contract: include/mico_hip.h.
//
// attn_decode_kernel: one wave per (set, head, key split, query chunk).  A set's keys are streamed once for all its queries
// (beams x positions per row), 64 keys per block:
//   scores   lane = key: the key's 64 dims (8 x 16 B loads) against every query held fp32 in LDS (broadcast reads);
//   softmax  online per query (wave max / sum), probabilities of the block to LDS as [query][key & 7][key >> 3];
//   P V      lane = (key group kg = lane >> 3, dims dg * 8 .. + 7): 8 keys x 16 B of V per lane, NQ x 8 fp32 accumulators;
//   end      the 8 key groups summed across lanes (fixed xor order), O / l written 16-bit - or, with a key split, the partial
//            (max, sum, o) of every query to the workspace, folded by attn_decode_combine_kernel in split order.
// Bound: HBM on the K/V stream (every key / value byte read once per (set, head)); fp32 VALU work = 4 NQ FMAs per key byte pair.
//
// Both kernels are templates over their argument block, and dec_set() is all that tells the two forms apart: with DecArgs every set owns
// R rows; with DecRaggedArgs (question answering: a sample's condition tokens are read by however many questions it has) set s owns the
// query rows [set_row0[s], set_row0[s + 1]) of a device table.  The ragged grid and workspace layout are sized by the largest set, and a
// workgroup beyond its set's chunk count leaves after reading the two table entries.  Per query the operations and their order do not
// depend on the form, so a ragged set's output equals the uniform launch over that set alone bit for bit.
#include "common.h"

namespace {

constexpr int DEC_HD = 64;     // head size (BERT-base); the host refuses any other
constexpr int DEC_QC = 4;      // queries per workgroup (a set with more queries runs ceil(QR / 4) query chunks): at 8 the fp32
                               // query / accumulator / prefetched K-V registers no longer fit and the kernel spills

struct DecArgs {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    const float* mask;
    float* ws;
    int64_t q_rs, kv_ss, kv_rs, o_rs, mask_rs, mask_qs;
    int R, Qp, QR, H, Sk, nchunk, splits, bps;
    float scale;
};

struct DecRaggedArgs : DecArgs {     // R / QR / nchunk: the LARGEST set's (grid and workspace layout)
    const int* set_row0;             // [sets + 1] ascending first-row table
};

struct DecSet {
    int q0;         // first query (row of q / o)
    int row0;       // first mask row
    int QR;         // queries
};

__device__ __forceinline__ DecSet dec_set(const DecArgs& a, int s) { return {s * a.QR, s * a.R, a.QR}; }
__device__ __forceinline__ DecSet dec_set(const DecRaggedArgs& a, int s) {
    const int row0 = a.set_row0[s];
    return {row0 * a.Qp, row0, (a.set_row0[s + 1] - row0) * a.Qp};      // (the host has checked that rows * Qp fits an int)
}

__device__ __forceinline__ float xor_lane_sum(float v, int m) { return v + __shfl_xor(v, m, 64); }

// Chunks are counted from the set's first query; the workspace is laid out at a.nchunk chunks per (set, head) (ragged: unused parts unwritten).
template <typename T, int NQ, typename Args>
__global__ __launch_bounds__(64) void attn_decode_kernel(Args a) {
    const int sh = blockIdx.x, sp = blockIdx.y, qc = blockIdx.z;
    const int s = sh / a.H, h = sh - s * a.H;
    const DecSet set = dec_set(a, s);
    const int g0 = qc * DEC_QC;
    // ragged only, compiled out of the uniform form (its grid has no such workgroup): before any barrier and any q / k / v / o access
    if (std::is_same<Args, DecRaggedArgs>::value && g0 >= set.QR) return;
    const int lane = threadIdx.x;
    const int nq = min(NQ, set.QR - g0);
    __shared__ float qs[NQ][DEC_HD];        // queries of the chunk, fp32 (padding rows 0)
    __shared__ float pl[NQ][8][8];          // probabilities of the current key block: [query][key & 7][key >> 3]
    int64_t moff[NQ];                       // mask row of each query (elements from a.mask)
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int g = g0 + (j < nq ? j : 0);
        const int r = g / a.Qp, qi = g - r * a.Qp;
        moff[j] = (int64_t)(set.row0 + r) * a.mask_rs + (int64_t)qi * a.mask_qs;
        float x = 0.f;
        if (j < nq) x = to_f32(((const T*)a.q)[(int64_t)(set.q0 + g) * a.q_rs + h * DEC_HD + lane]);
        qs[j][lane] = x;
    }
    __syncthreads();

    const int nblk = (a.Sk + 63) >> 6;
    const int b0 = sp * a.bps, b1 = min(nblk, b0 + a.bps);
    const T* kb = (const T*)a.k + (int64_t)s * a.kv_ss + h * DEC_HD;
    const T* vb = (const T*)a.v + (int64_t)s * a.kv_ss + h * DEC_HD;
    const int kg = lane >> 3, dg = lane & 7;
    float M[NQ], L[NQ], acc[NQ][8];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        M[j] = -INFINITY;
        L[j] = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[j][c] = 0.f;
    }
    for (int blk = b0; blk < b1; ++blk) {
        // ---- scores: lane = key
        const int key = (blk << 6) + lane;
        const bool valid = key < a.Sk;
        s16x8 kr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kr[i] = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
        if (valid) {
            const s16x8* kp = (const s16x8*)(kb + (int64_t)key * a.kv_rs);
#pragma unroll
            for (int i = 0; i < 8; ++i) kr[i] = kp[i];
        }
        float kf[DEC_HD];
#pragma unroll
        for (int i = 0; i < 8; ++i) unpack8<T>(kr[i], kf + i * 8);
        float sc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < DEC_HD; ++c) d = fmaf(qs[j][c], kf[c], d);
            sc[j] = d;
        }
        // ---- online softmax per query
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float x = -INFINITY;
            if (valid) x = sc[j] * a.scale + (a.mask ? a.mask[moff[j] + key] : 0.f);
            const float mn = fmaxf(M[j], wave_max(x));      // finite: a block holds at least one valid key
            const float al = __expf(M[j] - mn);
            const float p = __expf(x - mn);
            L[j] = L[j] * al + wave_sum(p);
            M[j] = mn;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[j][c] *= al;
            pl[j][lane & 7][lane >> 3] = p;
        }
        __syncthreads();
        // ---- P V: lane = (key group, 8 dims); keys i * 8 + kg of the block
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kk = (blk << 6) + i * 8 + kg;
            s16x8 vr = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (kk < a.Sk) vr = *(const s16x8*)(vb + (int64_t)kk * a.kv_rs + dg * 8);
            float vf[8];
            unpack8<T>(vr, vf);
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const float pj = pl[j][kg][i];
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[j][c] = fmaf(pj, vf[c], acc[j][c]);
            }
        }
        __syncthreads();
    }
    // ---- the 8 key groups of a dim slice: lanes dg, dg + 8, ..., dg + 56 (fixed order)
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float x = xor_lane_sum(acc[j][c], 8);
            x = xor_lane_sum(x, 16);
            acc[j][c] = xor_lane_sum(x, 32);
        }
    }
    if (kg != 0) return;
    if (a.splits == 1) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (j >= nq) continue;
            const float inv = 1.f / L[j];
            float ov[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) ov[c] = acc[j][c] * inv;
            *(s16x8*)((T*)a.o + (int64_t)(set.q0 + g0 + j) * a.o_rs + h * DEC_HD + dg * 8) = pack8<T>(ov);
        }
        return;
    }
    const int64_t part0 = ((int64_t)(sh * a.nchunk + qc) * a.splits + sp) * DEC_QC;
    const int64_t nparts = (int64_t)gridDim.x * a.nchunk * a.splits * DEC_QC;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        if (j >= nq) continue;
        float* po = a.ws + (part0 + j) * DEC_HD + dg * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) po[c] = acc[j][c];
        if (dg == 0) {
            a.ws[nparts * DEC_HD + (part0 + j) * 2] = M[j];
            a.ws[nparts * DEC_HD + (part0 + j) * 2 + 1] = L[j];
        }
    }
}

// partials of the key splits -> O: lane = dim; weights exp(m_s - max) summed in split order (bit-identical from run to run)
template <typename T, typename Args>
__global__ __launch_bounds__(64) void attn_decode_combine_kernel(Args a) {
    const int sh = blockIdx.x, qc = blockIdx.y;
    const int s = sh / a.H, h = sh - s * a.H;
    const DecSet set = dec_set(a, s);
    const int g0 = qc * DEC_QC;
    if (std::is_same<Args, DecRaggedArgs>::value && g0 >= set.QR) return;
    const int lane = threadIdx.x;
    const int nq = min(DEC_QC, set.QR - g0);
    const int64_t nparts = (int64_t)gridDim.x * a.nchunk * a.splits * DEC_QC;
    const float* ml = a.ws + nparts * DEC_HD;
    for (int j = 0; j < nq; ++j) {
        const int64_t p0 = (int64_t)(sh * a.nchunk + qc) * a.splits * DEC_QC + j;
        float mx = -INFINITY;
        for (int sp = 0; sp < a.splits; ++sp) mx = fmaxf(mx, ml[(p0 + sp * DEC_QC) * 2]);
        float l = 0.f, o = 0.f;
        for (int sp = 0; sp < a.splits; ++sp) {
            const int64_t p = p0 + sp * DEC_QC;
            const float w = __expf(ml[p * 2] - mx);
            l = fmaf(ml[p * 2 + 1], w, l);
            o = fmaf(a.ws[p * DEC_HD + lane], w, o);
        }
        ((T*)a.o)[(int64_t)(set.q0 + g0 + j) * a.o_rs + h * DEC_HD + lane] = from_f32<T>(o / l);
    }
}

// dst[r][pos0 + i][0 .. width) = src[r * n_new + i][0 .. width): 16-bit elements, 16 B per thread
__global__ __launch_bounds__(256) void decode_kv_append_kernel(const s16x8* __restrict__ src, int64_t src_rs8, s16x8* __restrict__ dst,
                                                               int64_t dst_ss8, int64_t dst_rs8, int n_new, int pos0, int width8) {
    const int row = blockIdx.x;                 // r * n_new + i
    const int r = row / n_new, i = row - r * n_new;
    const s16x8* s = src + (int64_t)row * src_rs8;
    s16x8* d = dst + (int64_t)r * dst_ss8 + (int64_t)(pos0 + i) * dst_rs8;
    for (int c = threadIdx.x; c < width8; c += blockDim.x) d[c] = s[c];
}

// dst[l][r][0 .. n) = src[l][parent[r]][0 .. n): the cache's first positions re-gathered by parent row; a parent outside [0, rows)
// leaves its row unwritten
__global__ __launch_bounds__(256) void decode_kv_gather_kernel(const s16x8* __restrict__ src, s16x8* __restrict__ dst,
                                                               const int64_t* __restrict__ parent, int rows, int64_t layer_stride8,
                                                               int64_t row_stride8, int64_t n8) {
    const int r = blockIdx.y, l = blockIdx.z;
    const int64_t pr = parent[r];
    if (pr < 0 || pr >= rows) return;
    const s16x8* s = src + l * layer_stride8 + pr * row_stride8;
    s16x8* d = dst + l * layer_stride8 + (int64_t)r * row_stride8;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n8; c += (int64_t)gridDim.x * blockDim.x) d[c] = s[c];
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct DecSplit {
    int bps;     // 64-key blocks per split
    int eff;     // splits that hold at least one block
};

inline DecSplit dec_split(int Sk, int splits) {
    const int nblk = (Sk + 63) / 64;
    const int sp = splits < nblk ? splits : nblk;
    const int bps = (nblk + sp - 1) / sp;
    return {bps, (nblk + bps - 1) / bps};
}

// Both entry points: fn is the caller's name (every error text starts with it).  ragged: set s owns the rows of set_row0, `rows` in all and
// R in the largest set; otherwise every set owns R rows (rows = sets * R, set_row0 unused).
int attn_decode(const char* fn, bool ragged, const void* q, int64_t q_rs, const void* k, const void* v, int64_t kv_ss, int64_t kv_rs, void* o,
                int64_t o_rs, const float* mask, int64_t mask_rs, int64_t mask_qs, int sets, const int* set_row0, int64_t rows, int R, int Qp,
                int H, int Sk, int hd, float scale, int splits, float* ws, int64_t ws_bytes, int dtype, void* stream) {
    MICO_CHECK(hd == DEC_HD, "%s: head size %d is not supported (hd 64 only)", fn, hd);
    MICO_CHECK(dtype_ok(dtype) && q && k && v && o && (set_row0 || !ragged), "%s: bad args", fn);
    const bool positive = sets >= 1 && rows >= 1 && R >= 1 && Qp >= 1 && H >= 1 && Sk >= 1 && splits >= 1;
    if (ragged) {
        MICO_CHECK(positive, "%s: sets %d rows %d max_rows_per_set %d q_per_row %d H %d Sk %d splits %d must be positive", fn, sets, (int)rows,
                   R, Qp, H, Sk, splits);
        MICO_CHECK(R <= rows && (int64_t)sets * R >= rows, "%s: %d rows cannot be %d sets of at most %d rows", fn, (int)rows, sets, R);
    } else {
        MICO_CHECK(positive, "%s: sets %d rows_per_set %d q_per_row %d H %d Sk %d splits %d must be positive", fn, sets, R, Qp, H, Sk, splits);
    }
    MICO_CHECK(al16(q) && al16(k) && al16(v) && al16(o) && q_rs % 8 == 0 && kv_rs % 8 == 0 && kv_ss % 8 == 0 && o_rs % 8 == 0,
               "%s: q / k / v / o and their strides must be 16-byte aligned", fn);
    MICO_CHECK(q_rs >= (int64_t)H * hd && o_rs >= (int64_t)H * hd && kv_rs >= (int64_t)H * hd, "%s: row strides below H * hd", fn);
    MICO_CHECK((int64_t)sets * H < 0x7fffffff && rows * Qp < 0x7fffffff, "%s: too many queries", fn);
    const int QR = R * Qp;      // (R <= rows: fits)
    const DecSplit ks = dec_split(Sk, splits);
    const int nchunk = (QR + DEC_QC - 1) / DEC_QC;
    MICO_CHECK(nchunk <= 65535 && ks.eff <= 65535, "%s: grid too large", fn);
    if (ks.eff > 1) {
        const int need = mico_attn_decode_ws_bytes(sets, H, QR, Sk, splits);
        MICO_CHECK(need > 0 && ws && ws_bytes >= need, "%s: a %d-way key split needs a %d-byte fp32 workspace (got %lld)", fn, ks.eff, need,
                   (long long)ws_bytes);
    }
    DecRaggedArgs a;
    a.q = q; a.k = k; a.v = v; a.o = o; a.mask = mask; a.ws = ws;
    a.q_rs = q_rs; a.kv_ss = kv_ss; a.kv_rs = kv_rs; a.o_rs = o_rs; a.mask_rs = mask_rs; a.mask_qs = mask_qs;
    a.R = R; a.Qp = Qp; a.QR = QR; a.H = H; a.Sk = Sk; a.nchunk = nchunk; a.splits = ks.eff; a.bps = ks.bps;
    a.scale = scale; a.set_row0 = set_row0;
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](const auto& args) -> int {       // args: the kernels' argument block, DecArgs or DecRaggedArgs
        typedef std::decay_t<decltype(args)> Args;
        const dim3 grid(sets * H, ks.eff, nchunk);
        DISPATCH_T16(dtype, {
            if (QR <= 2) MICO_LAUNCH((attn_decode_kernel<T, 2, Args>), grid, dim3(64), 0, st, args);
            else MICO_LAUNCH((attn_decode_kernel<T, 4, Args>), grid, dim3(64), 0, st, args);
        });
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && ks.eff > 1) {
            DISPATCH_T16(dtype, MICO_LAUNCH((attn_decode_combine_kernel<T, Args>), dim3(sets * H, nchunk), dim3(64), 0, st, args));
            e = hipGetLastError();
        }
        return e == hipSuccess ? 0 : mico_set_err(MICO_ELAUNCH, "%s: %s", fn, hipGetErrorString(e));
    };
    return ragged ? launch(a) : launch(static_cast<const DecArgs&>(a));
}

}  // namespace

extern "C" int mico_attn_decode_ws_bytes(int sets, int H, int QR, int Sk, int splits) {
    if (sets < 1 || H < 1 || QR < 1 || Sk < 1 || splits < 1) return -1;
    const int eff = dec_split(Sk, splits).eff;
    if (eff == 1) return 0;
    const int64_t n = (int64_t)sets * H * ((QR + DEC_QC - 1) / DEC_QC) * eff * DEC_QC * (DEC_HD + 2) * 4;
    return n > 0x7fffffff ? -1 : (int)n;
}

extern "C" int mico_attn_decode(const void* q, int64_t q_rs, const void* k, const void* v, int64_t kv_ss, int64_t kv_rs, void* o,
                                int64_t o_rs, const float* mask, int64_t mask_rs, int64_t mask_qs, int sets, int rows_per_set,
                                int q_per_row, int H, int Sk, int hd, float scale, int splits, float* ws, int64_t ws_bytes,
                                int dtype, void* stream) {
    return attn_decode("mico_attn_decode", false, q, q_rs, k, v, kv_ss, kv_rs, o, o_rs, mask, mask_rs, mask_qs, sets, nullptr,
                       (int64_t)sets * rows_per_set, rows_per_set, q_per_row, H, Sk, hd, scale, splits, ws, ws_bytes, dtype, stream);
}

extern "C" int mico_attn_decode_ragged_ws_bytes(int sets, int H, int max_rows_per_set, int q_per_row, int Sk, int splits) {
    if (max_rows_per_set < 1 || q_per_row < 1 || (int64_t)max_rows_per_set * q_per_row > 0x7fffffff) return -1;
    return mico_attn_decode_ws_bytes(sets, H, max_rows_per_set * q_per_row, Sk, splits);
}

extern "C" int mico_attn_decode_ragged(const void* q, int64_t q_rs, const void* k, const void* v, int64_t kv_ss, int64_t kv_rs, void* o,
                                       int64_t o_rs, const float* mask, int64_t mask_rs, int64_t mask_qs, int sets, const int* set_row0,
                                       int rows, int max_rows_per_set, int q_per_row, int H, int Sk, int hd, float scale, int splits,
                                       float* ws, int64_t ws_bytes, int dtype, void* stream) {
    return attn_decode("mico_attn_decode_ragged", true, q, q_rs, k, v, kv_ss, kv_rs, o, o_rs, mask, mask_rs, mask_qs, sets, set_row0, rows,
                       max_rows_per_set, q_per_row, H, Sk, hd, scale, splits, ws, ws_bytes, dtype, stream);
}

extern "C" int mico_decode_kv_append(const void* src, int64_t src_rs, void* cache, int64_t cache_ss, int64_t cache_rs, int rows,
                                     int n_new, int pos0, int width, void* stream) {
    MICO_CHECK(src && cache && rows >= 1 && n_new >= 1 && pos0 >= 0 && width >= 8, "mico_decode_kv_append: bad args");
    MICO_CHECK(al16(src) && al16(cache) && src_rs % 8 == 0 && cache_ss % 8 == 0 && cache_rs % 8 == 0 && width % 8 == 0,
               "mico_decode_kv_append: 16-bit operands, 16-byte aligned rows and widths");
    MICO_CHECK((int64_t)rows * n_new < 0x7fffffff && cache_rs >= width && cache_ss >= (int64_t)(pos0 + n_new) * cache_rs,
               "mico_decode_kv_append: positions %d .. %d do not fit the cache rows", pos0, pos0 + n_new - 1);
    MICO_LAUNCH(decode_kv_append_kernel, dim3(rows * n_new), dim3(256), 0, (hipStream_t)stream, (const s16x8*)src, src_rs / 8,
                (s16x8*)cache, cache_ss / 8, cache_rs / 8, n_new, pos0, width / 8);
    MICO_LAUNCH_CHECK();
    return 0;
}

extern "C" int mico_decode_kv_gather(const void* src, void* dst, const int64_t* parent, int layers, int rows, int64_t layer_stride,
                                     int64_t row_stride, int64_t n, void* stream) {
    MICO_CHECK(src && dst && parent && src != dst && layers >= 1 && rows >= 1 && n >= 0, "mico_decode_kv_gather: bad args");
    MICO_CHECK(al16(src) && al16(dst) && layer_stride % 8 == 0 && row_stride % 8 == 0 && n % 8 == 0 && n <= row_stride &&
               layer_stride >= (int64_t)rows * row_stride && layers <= 65535 && rows <= 65535,
               "mico_decode_kv_gather: 16-bit operands, 16-byte aligned rows, n within a row");
    if (n == 0) return 0;
    const int64_t n8 = n / 8;
    const int gx = (int)((n8 + 255) / 256 < 64 ? (n8 + 255) / 256 : 64);
    MICO_LAUNCH(decode_kv_gather_kernel, dim3(gx, rows, layers), dim3(256), 0, (hipStream_t)stream, (const s16x8*)src, (s16x8*)dst,
                parent, rows, layer_stride / 8, row_stride / 8, n8);
    MICO_LAUNCH_CHECK();
    return 0;
}
