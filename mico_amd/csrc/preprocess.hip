// Batched crop / resize / flip / normalise of decoded frames (include/mico_hip.h, "Batched crop / resize / flip / normalise"): one launch for a
// ragged batch of uint8 RGB frames, every frame described by one row of a device int64 table.  The crop box, the virtual resize, the output
// window and the flip are folded into the sampling arithmetic; nothing is copied in between.
#include "common.h"

namespace {

constexpr int AUG_COLS = 12;   // int64 columns per table row: off, pitch, top, left, ch, cw, rh, rw, oy, ox, flip, reserved
constexpr int AUG_RUN = 4;     // horizontally adjacent output pixels per thread

// The two horizontally adjacent taps (columns x0 and x0 + 1, six contiguous bytes from byte `a` of src) as packed 0x00BBGGRR words.  `a` is
// clamped into the buffer first.  Fast path: three aligned dwords that cover a .. a + 5 and two v_alignbyte (a frame may start at any byte,
// so a tap is never known to be dword-aligned); it needs src itself dword-aligned (dw_ok) and the dwords inside the buffer.  Near the end
// of the buffer: six byte loads, each address clamped.  two == false (x1 == x0, the region's right edge): the second tap IS the first.
__device__ __forceinline__ void load_taps(const unsigned char* __restrict__ src, int64_t nbytes, int64_t a, bool two, bool dw_ok,
                                          unsigned& p0, unsigned& p1) {
    const int64_t last = nbytes - 1;
    a = a < 0 ? 0 : (a > last ? last : a);
    const int64_t base = a & ~(int64_t)3;
    if (dw_ok && base + 12 <= nbytes) {
        const unsigned* q = (const unsigned*)(src + base);
        const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
        const unsigned sh = (unsigned)a & 3u;
        const unsigned w0 = __builtin_amdgcn_alignbyte(d1, d0, sh), w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);   // bytes a .. a+3, a+4 .. a+7
        p0 = w0 & 0xffffffu;
        p1 = (w0 >> 24) | ((w1 & 0xffffu) << 8);
    } else {
        unsigned b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int64_t ai = a + i;
            b[i] = src[ai > last ? last : ai];
        }
        p0 = b[0] | (b[1] << 8) | (b[2] << 16);
        p1 = b[3] | (b[4] << 8) | (b[5] << 16);
    }
    if (!two) p1 = p0;
}

// grid.x covers the out_h * ceil(out_w / 4) runs of one frame, grid.y walks the frames: the table row is the same for a whole workgroup, so
// it is read through the scalar cache.  Consecutive lanes own consecutive runs of a row: a wave's stores to a plane are contiguous along x.
template <bool VEC>
__global__ __launch_bounds__(256) void image_augment_kernel(const unsigned char* __restrict__ src, int64_t nbytes,
                                                            const int64_t* __restrict__ table, int n, float* __restrict__ dst, int oh, int ow,
                                                            float m0, float m1, float m2, float s0, float s1, float s2, int dw_ok) {
    const int G = (ow + AUG_RUN - 1) / AUG_RUN;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= oh * G) return;
    const int y = item / G, xb = (item - y * G) * AUG_RUN;
    const float mean[3] = {m0, m1, m2}, istd[3] = {s0, s1, s2};
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const int64_t* t = table + (int64_t)f * AUG_COLS;
        const uint64_t off = (uint64_t)t[0], pitch = (uint64_t)t[1];   // unsigned: a nonsense table wraps instead of overflowing, then clamps
        const int top = (int)t[2], left = (int)t[3], ch = (int)t[4], cw = (int)t[5], rh = (int)t[6], rw = (int)t[7];
        const int oy = (int)t[8], ox = (int)t[9];
        const bool flip = t[10] != 0;
        const float sy = (float)ch / (float)rh, sx = (float)cw / (float)rw;

        float fy = sy * ((float)(y + oy) + 0.5f) - 0.5f;
        fy = fy < 0.f ? 0.f : fy;
        const int y0 = (int)fy;
        const int y1 = min(y0 + 1, ch - 1);
        const float ly = fy - (float)y0, hy = 1.f - ly;
        const uint64_t row0 = off + (uint64_t)(int64_t)(top + y0) * pitch, row1 = off + (uint64_t)(int64_t)(top + y1) * pitch;

        float out[3][AUG_RUN];
        int px0 = -1, px1 = -1;                   // the previous pixel's tap columns: equal columns (upsampling) reuse its four taps
        unsigned p00 = 0, p01 = 0, p10 = 0, p11 = 0;
#pragma unroll
        for (int j = 0; j < AUG_RUN; ++j) {
            const int x = min(xb + j, ow - 1);    // a run that ends past out_w recomputes the last pixel and does not store it
            const int xs = flip ? ow - 1 - x : x;
            float fx = sx * ((float)(xs + ox) + 0.5f) - 0.5f;
            fx = fx < 0.f ? 0.f : fx;
            const int x0 = (int)fx;
            const int x1 = min(x0 + 1, cw - 1);
            const float lx = fx - (float)x0, hx = 1.f - lx;
            if (x0 != px0 || x1 != px1) {
                const uint64_t col = (uint64_t)(int64_t)(left + x0) * 3u;
                load_taps(src, nbytes, (int64_t)(row0 + col), x1 == x0 + 1, dw_ok != 0, p00, p01);
                load_taps(src, nbytes, (int64_t)(row1 + col), x1 == x0 + 1, dw_ok != 0, p10, p11);
                px0 = x0;
                px1 = x1;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float k = 1.f / 255.f;
                const float t00 = (float)((p00 >> (8 * c)) & 255u), t01 = (float)((p01 >> (8 * c)) & 255u);
                const float t10 = (float)((p10 >> (8 * c)) & 255u), t11 = (float)((p11 >> (8 * c)) & 255u);
                const float v = hy * (hx * (t00 * k) + lx * (t01 * k)) + ly * (hx * (t10 * k) + lx * (t11 * k));
                out[c][j] = (v - mean[c]) * istd[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = dst + (((int64_t)f * 3 + c) * oh + y) * ow + xb;
            if (VEC) {
                *(f32x4*)o = (f32x4){out[c][0], out[c][1], out[c][2], out[c][3]};
            } else {
#pragma unroll
                for (int j = 0; j < AUG_RUN; ++j)
                    if (xb + j < ow) o[j] = out[c][j];
            }
        }
    }
}

}  // namespace

extern "C" int mico_image_augment(const unsigned char* src, int64_t src_bytes, const int64_t* table, int n, float* dst, int out_h, int out_w,
                                  float mean0, float mean1, float mean2, float istd0, float istd1, float istd2, void* stream) {
    MICO_CHECK(src && table && dst, "mico_image_augment: null pointer");
    MICO_CHECK(n > 0 && src_bytes > 0 && out_h > 0 && out_w > 0, "mico_image_augment: n, src_bytes, out_h and out_w must be positive");
    MICO_CHECK((((uintptr_t)table) & 7) == 0, "mico_image_augment: table must be 8-byte aligned");
    const int64_t runs = (int64_t)out_h * ((out_w + AUG_RUN - 1) / AUG_RUN);
    MICO_CHECK(runs <= 0x7fffff00, "mico_image_augment: output too large");
    const dim3 grid((unsigned)((runs + 255) / 256), (unsigned)(n < 65535 ? n : 65535));
    const int dw_ok = (((uintptr_t)src) & 3) == 0;
    const bool vec = out_w % 4 == 0 && (((uintptr_t)dst) & 15) == 0;
    if (vec)
        MICO_LAUNCH(image_augment_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, src_bytes, table, n, dst, out_h, out_w, mean0, mean1,
                    mean2, istd0, istd1, istd2, dw_ok);
    else
        MICO_LAUNCH(image_augment_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, src_bytes, table, n, dst, out_h, out_w, mean0, mean1,
                    mean2, istd0, istd1, istd2, dw_ok);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}
