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
// attn_decode_ragged_kernel: the same wave program for sets that own DIFFERENT numbers of rows (question answering: a sample's condition
// tokens are read by however many questions it has).  Set s owns the query rows [set_row0[s], set_row0[s + 1]) of a device table; the
// grid is sized by the largest set, and a workgroup beyond its set's chunk count leaves after reading the two table entries.  It is a
// separate kernel so that the uniform instantiations above stay exactly as they were; per query it issues the same operations in the
// same order, so a set's output equals the uniform launch over that set alone bit for bit.
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

__device__ __forceinline__ float xor_lane_sum(float v, int m) { return v + __shfl_xor(v, m, 64); }

template <typename T, int NQ>
__global__ __launch_bounds__(64) void attn_decode_kernel(DecArgs a) {
    const int sh = blockIdx.x, sp = blockIdx.y, qc = blockIdx.z;
    const int s = sh / a.H, h = sh - s * a.H;
    const int lane = threadIdx.x;
    const int g0 = qc * DEC_QC;
    const int nq = min(NQ, a.QR - g0);
    __shared__ float qs[NQ][DEC_HD];        // queries of the chunk, fp32 (padding rows 0)
    __shared__ float pl[NQ][8][8];          // probabilities of the current key block: [query][key & 7][key >> 3]
    int64_t moff[NQ];                       // mask row of each query (elements from a.mask)
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int g = g0 + (j < nq ? j : 0);
        const int r = g / a.Qp, qi = g - r * a.Qp;
        moff[j] = (int64_t)(s * a.R + r) * a.mask_rs + (int64_t)qi * a.mask_qs;
        float x = 0.f;
        if (j < nq) x = to_f32(((const T*)a.q)[(int64_t)(s * a.QR + g) * a.q_rs + h * DEC_HD + lane]);
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
            *(s16x8*)((T*)a.o + (int64_t)(s * a.QR + g0 + j) * a.o_rs + h * DEC_HD + dg * 8) = pack8<T>(ov);
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
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_combine_kernel(DecArgs a) {
    const int sh = blockIdx.x, qc = blockIdx.y;
    const int s = sh / a.H, h = sh - s * a.H;
    const int lane = threadIdx.x;
    const int g0 = qc * DEC_QC;
    const int nq = min(DEC_QC, a.QR - g0);
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
        ((T*)a.o)[(int64_t)(s * a.QR + g0 + j) * a.o_rs + h * DEC_HD + lane] = from_f32<T>(o / l);
    }
}

struct DecRaggedArgs {
    DecArgs d;               // R / QR / nchunk: the LARGEST set's (grid and workspace layout); the others as in the uniform launch
    const int* set_row0;     // [sets + 1] ascending first-row table
};

// attn_decode_kernel for ragged sets: R, QR and the first query come from the table, everything else is the uniform program.  Chunks are
// counted from the set's first query; the workspace keeps the uniform layout at the largest set's chunk count (unused parts unwritten).
template <typename T, int NQ>
__global__ __launch_bounds__(64) void attn_decode_ragged_kernel(DecRaggedArgs ra) {
    const DecArgs& a = ra.d;
    const int sh = blockIdx.x, sp = blockIdx.y, qc = blockIdx.z;
    const int s = sh / a.H, h = sh - s * a.H;
    const int row0 = ra.set_row0[s];
    const int QR = (ra.set_row0[s + 1] - row0) * a.Qp;
    const int g0 = qc * DEC_QC;
    if (g0 >= QR) return;                   // (uniform for the workgroup: before any barrier, before any q / k / v / o access)
    const int64_t q0 = (int64_t)row0 * a.Qp;
    const int lane = threadIdx.x;
    const int nq = min(NQ, QR - g0);
    __shared__ float qs[NQ][DEC_HD];
    __shared__ float pl[NQ][8][8];
    int64_t moff[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int g = g0 + (j < nq ? j : 0);
        const int r = g / a.Qp, qi = g - r * a.Qp;
        moff[j] = (int64_t)(row0 + r) * a.mask_rs + (int64_t)qi * a.mask_qs;
        float x = 0.f;
        if (j < nq) x = to_f32(((const T*)a.q)[(q0 + g) * a.q_rs + h * DEC_HD + lane]);
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
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float x = -INFINITY;
            if (valid) x = sc[j] * a.scale + (a.mask ? a.mask[moff[j] + key] : 0.f);
            const float mn = fmaxf(M[j], wave_max(x));
            const float al = __expf(M[j] - mn);
            const float p = __expf(x - mn);
            L[j] = L[j] * al + wave_sum(p);
            M[j] = mn;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[j][c] *= al;
            pl[j][lane & 7][lane >> 3] = p;
        }
        __syncthreads();
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
            *(s16x8*)((T*)a.o + (q0 + g0 + j) * a.o_rs + h * DEC_HD + dg * 8) = pack8<T>(ov);
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

// attn_decode_combine_kernel for ragged sets (same fold, same order)
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_ragged_combine_kernel(DecRaggedArgs ra) {
    const DecArgs& a = ra.d;
    const int sh = blockIdx.x, qc = blockIdx.y;
    const int s = sh / a.H, h = sh - s * a.H;
    const int row0 = ra.set_row0[s];
    const int QR = (ra.set_row0[s + 1] - row0) * a.Qp;
    const int g0 = qc * DEC_QC;
    if (g0 >= QR) return;
    const int64_t q0 = (int64_t)row0 * a.Qp;
    const int lane = threadIdx.x;
    const int nq = min(DEC_QC, QR - g0);
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
        ((T*)a.o)[(q0 + g0 + j) * a.o_rs + h * DEC_HD + lane] = from_f32<T>(o / l);
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

}  // namespace

extern "C" int mico_attn_decode_ws_bytes(int sets, int H, int QR, int Sk, int splits) {
    if (sets < 1 || H < 1 || QR < 1 || Sk < 1 || splits < 1) return -1;
    const int nblk = (Sk + 63) / 64;
    const int sp = splits < nblk ? splits : nblk;
    const int bps = (nblk + sp - 1) / sp;
    const int eff = (nblk + bps - 1) / bps;
    if (eff == 1) return 0;
    const int64_t n = (int64_t)sets * H * ((QR + DEC_QC - 1) / DEC_QC) * eff * DEC_QC * (DEC_HD + 2) * 4;
    return n > 0x7fffffff ? -1 : (int)n;
}

extern "C" int mico_attn_decode(const void* q, int64_t q_rs, const void* k, const void* v, int64_t kv_ss, int64_t kv_rs, void* o,
                                int64_t o_rs, const float* mask, int64_t mask_rs, int64_t mask_qs, int sets, int rows_per_set,
                                int q_per_row, int H, int Sk, int hd, float scale, int splits, float* ws, int64_t ws_bytes,
                                int dtype, void* stream) {
    MICO_CHECK(hd == DEC_HD, "mico_attn_decode: head size %d is not supported (hd 64 only)", hd);
    MICO_CHECK(dtype_ok(dtype) && q && k && v && o, "mico_attn_decode: bad args");
    MICO_CHECK(sets >= 1 && rows_per_set >= 1 && q_per_row >= 1 && H >= 1 && Sk >= 1 && splits >= 1,
               "mico_attn_decode: sets %d rows_per_set %d q_per_row %d H %d Sk %d splits %d must be positive", sets, rows_per_set,
               q_per_row, H, Sk, splits);
    MICO_CHECK(al16(q) && al16(k) && al16(v) && al16(o) && q_rs % 8 == 0 && kv_rs % 8 == 0 && kv_ss % 8 == 0 && o_rs % 8 == 0,
               "mico_attn_decode: q / k / v / o and their strides must be 16-byte aligned");
    MICO_CHECK(q_rs >= (int64_t)H * hd && o_rs >= (int64_t)H * hd && kv_rs >= (int64_t)H * hd, "mico_attn_decode: row strides below H * hd");
    const int64_t QR = (int64_t)rows_per_set * q_per_row;
    MICO_CHECK((int64_t)sets * H < 0x7fffffff && QR * sets < 0x7fffffff, "mico_attn_decode: too many queries");
    const int nblk = (Sk + 63) / 64;
    const int sp = splits < nblk ? splits : nblk;
    const int bps = (nblk + sp - 1) / sp;
    const int eff = (nblk + bps - 1) / bps;
    const int nchunk = (int)((QR + DEC_QC - 1) / DEC_QC);
    MICO_CHECK(nchunk <= 65535 && eff <= 65535, "mico_attn_decode: grid too large");
    if (eff > 1) {
        const int need = mico_attn_decode_ws_bytes(sets, H, (int)QR, Sk, splits);
        MICO_CHECK(need > 0 && ws && ws_bytes >= need, "mico_attn_decode: a %d-way key split needs a %d-byte fp32 workspace (got %lld)",
                   eff, need, (long long)ws_bytes);
    }
    DecArgs a;
    a.q = q; a.k = k; a.v = v; a.o = o; a.mask = mask; a.ws = ws;
    a.q_rs = q_rs; a.kv_ss = kv_ss; a.kv_rs = kv_rs; a.o_rs = o_rs; a.mask_rs = mask_rs; a.mask_qs = mask_qs;
    a.R = rows_per_set; a.Qp = q_per_row; a.QR = (int)QR; a.H = H; a.Sk = Sk; a.nchunk = nchunk; a.splits = eff; a.bps = bps;
    a.scale = scale;
    const int nq = QR < DEC_QC ? (int)QR : DEC_QC;
    const dim3 grid(sets * H, eff, nchunk);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T16(dtype, {
        if (nq <= 2) MICO_LAUNCH((attn_decode_kernel<T, 2>), grid, dim3(64), 0, st, a);
        else MICO_LAUNCH((attn_decode_kernel<T, 4>), grid, dim3(64), 0, st, a);
    });
    MICO_LAUNCH_CHECK();
    if (eff > 1) {
        DISPATCH_T16(dtype, MICO_LAUNCH((attn_decode_combine_kernel<T>), dim3(sets * H, nchunk), dim3(64), 0, st, a));
        MICO_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mico_attn_decode_ragged_ws_bytes(int sets, int H, int max_rows_per_set, int q_per_row, int Sk, int splits) {
    if (max_rows_per_set < 1 || q_per_row < 1 || (int64_t)max_rows_per_set * q_per_row > 0x7fffffff) return -1;
    return mico_attn_decode_ws_bytes(sets, H, max_rows_per_set * q_per_row, Sk, splits);
}

extern "C" int mico_attn_decode_ragged(const void* q, int64_t q_rs, const void* k, const void* v, int64_t kv_ss, int64_t kv_rs, void* o,
                                       int64_t o_rs, const float* mask, int64_t mask_rs, int64_t mask_qs, int sets, const int* set_row0,
                                       int rows, int max_rows_per_set, int q_per_row, int H, int Sk, int hd, float scale, int splits,
                                       float* ws, int64_t ws_bytes, int dtype, void* stream) {
    MICO_CHECK(hd == DEC_HD, "mico_attn_decode_ragged: head size %d is not supported (hd 64 only)", hd);
    MICO_CHECK(dtype_ok(dtype) && q && k && v && o && set_row0, "mico_attn_decode_ragged: bad args");
    MICO_CHECK(sets >= 1 && rows >= 1 && max_rows_per_set >= 1 && q_per_row >= 1 && H >= 1 && Sk >= 1 && splits >= 1,
               "mico_attn_decode_ragged: sets %d rows %d max_rows_per_set %d q_per_row %d H %d Sk %d splits %d must be positive", sets, rows,
               max_rows_per_set, q_per_row, H, Sk, splits);
    MICO_CHECK(max_rows_per_set <= rows && (int64_t)sets * max_rows_per_set >= rows,
               "mico_attn_decode_ragged: %d rows cannot be %d sets of at most %d rows", rows, sets, max_rows_per_set);
    MICO_CHECK(al16(q) && al16(k) && al16(v) && al16(o) && q_rs % 8 == 0 && kv_rs % 8 == 0 && kv_ss % 8 == 0 && o_rs % 8 == 0,
               "mico_attn_decode_ragged: q / k / v / o and their strides must be 16-byte aligned");
    MICO_CHECK(q_rs >= (int64_t)H * hd && o_rs >= (int64_t)H * hd && kv_rs >= (int64_t)H * hd,
               "mico_attn_decode_ragged: row strides below H * hd");
    const int64_t QR = (int64_t)max_rows_per_set * q_per_row;
    MICO_CHECK((int64_t)sets * H < 0x7fffffff && (int64_t)rows * q_per_row < 0x7fffffff, "mico_attn_decode_ragged: too many queries");
    const int nblk = (Sk + 63) / 64;
    const int sp = splits < nblk ? splits : nblk;
    const int bps = (nblk + sp - 1) / sp;
    const int eff = (nblk + bps - 1) / bps;
    const int nchunk = (int)((QR + DEC_QC - 1) / DEC_QC);
    MICO_CHECK(nchunk <= 65535 && eff <= 65535, "mico_attn_decode_ragged: grid too large");
    if (eff > 1) {
        const int need = mico_attn_decode_ragged_ws_bytes(sets, H, max_rows_per_set, q_per_row, Sk, splits);
        MICO_CHECK(need > 0 && ws && ws_bytes >= need,
                   "mico_attn_decode_ragged: a %d-way key split needs a %d-byte fp32 workspace (got %lld)", eff, need, (long long)ws_bytes);
    }
    DecRaggedArgs ra;
    DecArgs& a = ra.d;
    a.q = q; a.k = k; a.v = v; a.o = o; a.mask = mask; a.ws = ws;
    a.q_rs = q_rs; a.kv_ss = kv_ss; a.kv_rs = kv_rs; a.o_rs = o_rs; a.mask_rs = mask_rs; a.mask_qs = mask_qs;
    a.R = max_rows_per_set; a.Qp = q_per_row; a.QR = (int)QR; a.H = H; a.Sk = Sk; a.nchunk = nchunk; a.splits = eff; a.bps = bps;
    a.scale = scale;
    ra.set_row0 = set_row0;
    const dim3 grid(sets * H, eff, nchunk);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T16(dtype, {
        if (QR <= 2) MICO_LAUNCH((attn_decode_ragged_kernel<T, 2>), grid, dim3(64), 0, st, ra);
        else MICO_LAUNCH((attn_decode_ragged_kernel<T, 4>), grid, dim3(64), 0, st, ra);
    });
    MICO_LAUNCH_CHECK();
    if (eff > 1) {
        DISPATCH_T16(dtype, MICO_LAUNCH((attn_decode_ragged_combine_kernel<T>), dim3(sets * H, nchunk), dim3(64), 0, st, ra));
        MICO_LAUNCH_CHECK();
    }
    return 0;
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
