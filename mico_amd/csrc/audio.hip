// Audio front end on the device: sinc resampling to 16 kHz and the Kaldi log-mel filterbank (include/mico_hip.h, "Device-side audio front
// end").  Both restate torchaudio's published algorithms; every table arrives from the host, computed there in double precision.
#include "common.h"

namespace {

constexpr int FB_FRAME = 400;    // 25 ms at 16 kHz
constexpr int FB_SHIFT = 160;    // 10 ms
constexpr int FB_NC = 256;       // complex points of the packed 512-point real transform
// LDS image of a 256-entry array: entry i lives at word i + (i >> 5) (one pad word per 32).  ds_read_b32 / ds_write_b32 serve 32 lanes per
// cycle over 32 banks; the Stockham stages read at lane + 64 r (consecutive words) and write at 4 (lane - k) + k + r Ns, Ns = 1, 4, 16, 64 -
// the per-stage worst case of 32 lanes on one bank is 4 / 4 / 2 / 1 unpadded and 1 / 4 / 2 / 1 with the pad word (the stride-4 stage spreads
// over all banks; the stride-16 stage keeps its 4-way writes, a second skew that frees it makes the reads 2-way everywhere).
constexpr int FB_LD = FB_NC + FB_NC / 32;
__device__ __forceinline__ int fb_at(int i) { return i + (i >> 5); }
constexpr float FB_LOG_EPS = -15.942385f;   // logf(FLT_EPSILON), correctly rounded: the floor of step 7

// One wave per frame, four frames per 256-thread workgroup; the frame lives in registers (load .. window) and in the wave's own three LDS rows
// (FFT real / imaginary part, power spectrum) until its log-mel row is stored.  Waves past T recompute frame T - 1 and store nothing, so every
// wave meets every barrier.
__global__ __launch_bounds__(256) void kaldi_fbank_kernel(const mico_fbank_params p) {
    __shared__ float s_re[4][FB_LD], s_im[4][FB_LD], s_pw[4][FB_LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t frame = (int64_t)blockIdx.x * 4 + wv;
    const bool live = frame < p.T;
    const int64_t fi = live ? frame : (int64_t)p.T - 1;
    const int64_t start = p.frame_start ? p.frame_start[fi] : fi * FB_SHIFT;
    float* re = s_re[wv];
    float* im = s_im[wv];
    float* pw = s_pw[wv];

    // 1-2. samples j = lane + 64 i, scaled; frame mean
    float v[7], sum = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int j = lane + 64 * i;
        const int64_t g = start + j;
        v[i] = (j < FB_FRAME && g >= 0 && g < p.n_samples) ? p.wave[g] * p.scale : 0.f;
        sum += v[i];
    }
    const float mean = wave_sum(sum) / (float)FB_FRAME;
    // 3-4. pre-emphasis against the previous sample (lane - 1; lane 0 takes lane 63's previous register, sample 0 itself), Povey window;
    // sample j becomes the real (j even) or imaginary (j odd) part of complex point j / 2
    float carry = v[0];   // lane 0: x[j - 1] of its sample 64 i
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int j = lane + 64 * i;
        const float up = __shfl(v[i], (lane + 63) & 63);
        const float prev = lane == 0 ? carry : up;
        carry = up;
        if (j < FB_FRAME) {
            const float y = ((v[i] - mean) - 0.97f * (prev - mean)) * p.window[j];
            ((j & 1) ? im : re)[fb_at(j >> 1)] = y;
        }
    }
    if (lane < FB_NC - FB_FRAME / 2) {   // zero padding: samples 400..511
        re[fb_at(FB_FRAME / 2 + lane)] = 0.f;
        im[fb_at(FB_FRAME / 2 + lane)] = 0.f;
    }
    __syncthreads();

    // 5. 256-point complex FFT: four radix-4 Stockham stages (autosort: natural order in, natural order out), one butterfly per lane and stage
    const f32x2* tw = (const f32x2*)p.twiddle;   // tw[m] = (cos, -sin)(2 pi m / 512)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int Ns = 1 << (2 * s);
        const int k = lane & (Ns - 1);
        float ur[4], ui[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ur[r] = re[fb_at(lane + 64 * r)];
            ui[r] = im[fb_at(lane + 64 * r)];
        }
        if (s > 0) {
            const int step = k * (128 >> (2 * s));   // W_{4 Ns}^{r k} = W_512^{r k 128 / Ns}
#pragma unroll
            for (int r = 1; r < 4; ++r) {
                const f32x2 w = tw[r * step];
                const float xr = ur[r] * w[0] - ui[r] * w[1], xi = ur[r] * w[1] + ui[r] * w[0];
                ur[r] = xr;
                ui[r] = xi;
            }
        }
        const float a0r = ur[0] + ur[2], a0i = ui[0] + ui[2], a1r = ur[0] - ur[2], a1i = ui[0] - ui[2];
        const float a2r = ur[1] + ur[3], a2i = ui[1] + ui[3];
        const float a3r = ui[1] - ui[3], a3i = -(ur[1] - ur[3]);   // -i (u1 - u3)
        const int j0 = ((lane - k) << 2) + k;
        __syncthreads();
        re[fb_at(j0)] = a0r + a2r;          im[fb_at(j0)] = a0i + a2i;
        re[fb_at(j0 + Ns)] = a1r + a3r;     im[fb_at(j0 + Ns)] = a1i + a3i;
        re[fb_at(j0 + 2 * Ns)] = a0r - a2r; im[fb_at(j0 + 2 * Ns)] = a0i - a2i;
        re[fb_at(j0 + 3 * Ns)] = a1r - a3r; im[fb_at(j0 + 3 * Ns)] = a1i - a3i;
        __syncthreads();
    }
    // split step: X[k] = E + W_512^k O, E = (Z[k] + conj Z[256 - k]) / 2, O = (Z[k] - conj Z[256 - k]) / 2i; power of bins 0..255
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane + 64 * i, kc = (FB_NC - k) & (FB_NC - 1);
        const float zr = re[fb_at(k)], zi = im[fb_at(k)], cr = re[fb_at(kc)], ci = -im[fb_at(kc)];
        const float er = 0.5f * (zr + cr), ei = 0.5f * (zi + ci);
        const float orr = 0.5f * (zi - ci), oi = -0.5f * (zr - cr);
        const f32x2 w = tw[k];
        const float xr = er + (orr * w[0] - oi * w[1]), xi = ei + (orr * w[1] + oi * w[0]);
        pw[fb_at(k)] = xr * xr + xi * xi;
    }
    __syncthreads();

    // 6-7. one lane per mel filter, bins in order; log with the FLT_EPSILON floor
    const bool resize = p.mel_out != p.mel;
    for (int b = lane; b < p.mel; b += 64) {
        const int first = p.filt_bins[2 * b], cnt = p.filt_bins[2 * b + 1];
        const float* w = p.filt_w + p.filt_off[b];
        float e = 0.f;
        for (int t = 0; t < cnt; ++t) e = fmaf(w[t], pw[fb_at(first + t)], e);
        const float val = e <= 1.1920929e-07f ? FB_LOG_EPS : logf(e);
        if (resize) re[b] = val;
        else if (live) p.out[frame * p.mel + b] = val;
    }
    if (!resize) return;
    // 8. bilinear resize along the mel axis (align_corners = False)
    __syncthreads();
    if (!live) return;
    const float ratio = (float)p.mel / (float)p.mel_out;
    for (int j = lane; j < p.mel_out; j += 64) {
        const float sp = fmaxf(ratio * ((float)j + 0.5f) - 0.5f, 0.f);
        const int i0 = min((int)sp, p.mel - 1), i1 = min(i0 + 1, p.mel - 1);
        const float w1 = sp - (float)i0, w0 = 1.f - w1;
        p.out[frame * p.mel_out + j] = w0 * re[i0] + w1 * re[i1];
    }
}

// One output per lane, 256 consecutive outputs per workgroup; their input span is staged in LDS once (neighbouring outputs overlap by
// K - orig samples), the taps of a lane's phase stream from global memory four at a time.
__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ taps, int ldt,
                                                            int orig, int P, int width, float* __restrict__ out, int64_t n_out, int span) {
    extern __shared__ float s_x[];
    const int64_t o0 = (int64_t)blockIdx.x * 256;
    const int64_t f0 = o0 / P;
    const int64_t base = f0 * orig - width;
    for (int i = threadIdx.x; i < span; i += 256) {
        const int64_t g = base + i;
        s_x[i] = (g >= 0 && g < n) ? x[g] : 0.f;
    }
    __syncthreads();
    const int64_t o = o0 + threadIdx.x;
    if (o >= n_out) return;
    const int64_t f = o / P;
    const int ph = (int)(o - f * P);
    const float* tp = taps + (int64_t)ph * ldt;
    const float* xs = s_x + (int)(f - f0) * orig;
    float acc = 0.f;
    for (int j = 0; j < ldt; j += 4) {
        const f32x4 t = *(const f32x4*)(tp + j);
        acc = fmaf(t[0], xs[j], acc);
        acc = fmaf(t[1], xs[j + 1], acc);
        acc = fmaf(t[2], xs[j + 2], acc);
        acc = fmaf(t[3], xs[j + 3], acc);
    }
    out[o] = acc;
}

}  // namespace

extern "C" int mico_kaldi_fbank(const mico_fbank_params* p, void* stream) {
    MICO_CHECK(p && p->wave && p->window && p->twiddle && p->filt_bins && p->filt_off && p->filt_w && p->out, "mico_kaldi_fbank: null pointer");
    MICO_CHECK(p->mel >= 1 && p->mel <= FB_NC && p->mel_out >= 1, "mico_kaldi_fbank: mel must be in 1..256, mel_out >= 1");
    MICO_CHECK(p->T >= 0 && p->n_samples >= 0, "mico_kaldi_fbank: bad sizes");
    if (!p->frame_start)
        MICO_CHECK(p->T == 0 || (int64_t)(p->T - 1) * FB_SHIFT + FB_FRAME <= p->n_samples, "mico_kaldi_fbank: T frames do not fit n_samples");
    MICO_CHECK((((uintptr_t)p->twiddle) & 7) == 0, "mico_kaldi_fbank: twiddle must be 8-byte aligned");
    if (p->T == 0) return MICO_OK;
    MICO_LAUNCH(kaldi_fbank_kernel, dim3((unsigned)((p->T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *p);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}

extern "C" int mico_fbank_params_layout(int* out, int n) {
#define OFF(F) (int)offsetof(mico_fbank_params, F)
    const int t[] = {(int)sizeof(mico_fbank_params), OFF(wave), OFF(n_samples), OFF(frame_start), OFF(T), OFF(scale), OFF(window),
                     OFF(twiddle), OFF(mel), OFF(mel_out), OFF(filt_bins), OFF(filt_off), OFF(filt_w), OFF(out), -1};
#undef OFF
    const int total = (int)(sizeof(t) / sizeof(t[0]));
    for (int i = 0; i < n && i < total; ++i) out[i] = t[i];
    return total;
}

extern "C" int mico_resample_sinc(const float* wave, int64_t n, const float* taps, int K, int ldt, int orig, int P, int width, float* out,
                                  int64_t n_out, void* stream) {
    MICO_CHECK(wave && taps && out && n >= 0, "mico_resample_sinc: bad args");
    MICO_CHECK(orig >= 1 && P >= 1 && width >= 0 && K == 2 * width + orig, "mico_resample_sinc: K must be 2 width + orig");
    MICO_CHECK(ldt >= K && ldt % 4 == 0 && (((uintptr_t)taps) & 15) == 0, "mico_resample_sinc: taps rows must be 16-byte aligned, ldt % 4 == 0, ldt >= K");
    MICO_CHECK(n_out == (n * P + orig - 1) / orig, "mico_resample_sinc: n_out must be ceil(P n / orig)");
    const int64_t span = (int64_t)(1 + 254 / P) * orig + ldt;
    MICO_CHECK(span * 4 <= 65536, "mico_resample_sinc: the input span of 256 outputs (%lld samples) does not fit 64 KiB of LDS", (long long)span);
    if (n_out == 0) return MICO_OK;
    MICO_CHECK((n_out + 255) / 256 <= 0x7fffffff, "mico_resample_sinc: too many outputs");
    MICO_LAUNCH(resample_sinc_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), (size_t)span * 4, (hipStream_t)stream, wave, n, taps, ldt,
                orig, P, width, out, n_out, (int)span);
    MICO_LAUNCH_CHECK();
    return MICO_OK;
}
