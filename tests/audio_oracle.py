"""numpy restatement of the audio front end (include/mico_hip.h, "Device-side audio front end"): torchaudio 2.x's
`compliance.kaldi.fbank(wave * 2**15, num_mel_bins=mel, sample_frequency=16000, frame_length=25, frame_shift=10)` and
`transforms.Resample(rate, 16000)` (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), written from the published algorithms and
independent of the product's table builders (mico_amd/model/audioprocessor.py).  torchaudio itself is not available to pin against.
Every function takes the dtype it computes in: np.float64 is the reference, np.float32 the same code in the product's precision (the
yardstick of the GPU gate).  A helper for tests/test_audio_frontend_cpu.py and tests/test_audio_frontend_gpu.py, not a test."""
import math

import numpy as np

FRAME, SHIFT, NFFT, RATE = 400, 160, 512, 16000
EPS = np.float32(1.1920929e-07)
LOG_EPS32 = np.float32(np.log(np.float64(EPS)))      # logf(FLT_EPSILON), correctly rounded: -15.942385


def num_frames(n):
    """snip_edges: whole frames only"""
    return 1 + (n - FRAME) // SHIFT if n >= FRAME else 0


def frame_starts(lengths):
    """first sample of every frame of clips packed back to back, and each clip's frame count"""
    starts, counts, base = [], [], 0
    for n in lengths:
        t = num_frames(n)
        starts += [base + i * SHIFT for i in range(t)]
        counts.append(t)
        base += n
    return np.asarray(starts, dtype=np.int64), counts


def povey_window(dtype=np.float64):
    j = np.arange(FRAME, dtype=dtype)
    two_pi = dtype(2 * math.pi)
    return ((dtype(0.5) - dtype(0.5) * np.cos(two_pi * j / dtype(FRAME - 1))) ** dtype(0.85)).astype(dtype)


def mel_scale(f, dtype):
    return dtype(1127.0) * np.log(dtype(1.0) + np.asarray(f, dtype=dtype) / dtype(700.0))


def mel_banks(mel, dtype=np.float64):
    """[mel, 257] triangular filters on FFT bins 0..256 (bin 256 weighs nothing)"""
    m_lo, m_hi = mel_scale(20.0, dtype), mel_scale(8000.0, dtype)
    d = (m_hi - m_lo) / dtype(mel + 1)
    b = np.arange(mel, dtype=dtype)[:, None]
    left = m_lo + b * d
    centre = left + d
    right = left + dtype(2.0) * d
    m_k = mel_scale(dtype(RATE / NFFT) * np.arange(NFFT // 2, dtype=dtype), dtype)[None, :]
    up = (m_k - left) / (centre - left)
    down = (right - m_k) / (right - centre)
    w = np.maximum(dtype(0.0), np.minimum(up, down)).astype(dtype)
    return np.concatenate([w, np.zeros((mel, 1), dtype=dtype)], axis=1)


def filter_ranges(banks):
    """(first bin, count) of every filter's non-zero weights (contiguous by construction); an empty filter is (0, 0)"""
    out = []
    for row in banks:
        nz = np.nonzero(row)[0]
        if len(nz) == 0:
            out.append((0, 0))
        else:
            assert nz[-1] - nz[0] + 1 == len(nz)
            out.append((int(nz[0]), len(nz)))
    return out


def empty_filters(mel):
    return {b for b, (_, c) in enumerate(filter_ranges(mel_banks(mel, np.float64))) if c == 0}


def fbank(wave, mel, dtype=np.float64, scale=32768.0, starts=None):
    """wave [n] in [-1, 1] -> log-mel [T, mel] in `dtype`.  starts: frame_starts() of a packed wave (default: one clip)."""
    x = np.asarray(wave).astype(dtype) * dtype(scale)
    if starts is None:
        starts = np.arange(num_frames(len(x)), dtype=np.int64) * SHIFT
    if len(starts) == 0:
        return np.zeros((0, mel), dtype=dtype)
    fr = x[np.asarray(starts)[:, None] + np.arange(FRAME)[None, :]]
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = (fr - dtype(0.97) * prev) * povey_window(dtype)[None, :]
    pad = np.zeros((fr.shape[0], NFFT), dtype=dtype)
    pad[:, :FRAME] = fr
    spec = np.fft.rfft(pad, axis=1)
    assert spec.real.dtype == dtype
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    e = power @ mel_banks(mel, dtype).T
    return np.log(np.maximum(e, dtype(EPS))).astype(dtype)


def mel_resize(fb, mel_out, dtype=np.float64):
    """F.interpolate(fb[None, None], size=(T, mel_out), mode="bilinear", align_corners=False)[0, 0]: the T axis is the identity"""
    fb = np.asarray(fb).astype(dtype)
    mel = fb.shape[1]
    if mel_out == mel:
        return fb
    s = np.maximum((np.arange(mel_out, dtype=dtype) + dtype(0.5)) * (dtype(mel) / dtype(mel_out)) - dtype(0.5), dtype(0.0))
    i0 = np.minimum(np.floor(s).astype(np.int64), mel - 1)
    i1 = np.minimum(i0 + 1, mel - 1)
    w1 = (s - i0.astype(dtype))[None, :]
    return ((dtype(1.0) - w1) * fb[:, i0] + w1 * fb[:, i1]).astype(dtype)


def resample_taps(rate, new_rate=RATE):
    """(taps [P, K] fp64, orig, P, width) of Resample(rate, new_rate)"""
    g = math.gcd(int(rate), int(new_rate))
    orig, P = int(rate) // g, int(new_rate) // g
    base = min(orig, P) * 0.99
    width = math.ceil(6 * orig / base)
    j = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -P, -1, dtype=np.float64)[:, None] / P + j) * base
    t = np.clip(t, -6.0, 6.0)
    win = np.cos(t * math.pi / 6.0 / 2.0) ** 2
    t = t * math.pi
    safe = np.where(t == 0.0, 1.0, t)
    taps = np.where(t == 0.0, 1.0, np.sin(safe) / safe) * win * (base / orig)
    return taps, orig, P, width


def resample_len(n, rate, new_rate=RATE):
    g = math.gcd(int(rate), int(new_rate))
    orig, P = int(rate) // g, int(new_rate) // g
    return -((-P * n) // orig)


def resample(wave, rate, dtype=np.float64, new_rate=RATE):
    """pad (width, width + orig), correlate with every phase at stride orig, interleave the phases, cut to ceil(P n / orig)"""
    taps, orig, P, width = resample_taps(rate, new_rate)
    x = np.asarray(wave).astype(dtype)
    n = len(x)
    K = taps.shape[1]
    xp = np.concatenate([np.zeros(width, dtype=dtype), x, np.zeros(width + orig, dtype=dtype)])
    F = (len(xp) - K) // orig + 1
    fr = xp[(np.arange(F) * orig)[:, None] + np.arange(K)[None, :]]
    out = (fr @ taps.astype(dtype).T).reshape(-1)
    return out[:resample_len(n, rate, new_rate)].astype(dtype)


def windows(fb, idx, target_length, mean, std):
    """audioprocessor.py:45-62 in fp64: normalise by (mean, 2 std), zero-pad to whole windows, pick the windows idx"""
    fb = (np.asarray(fb, dtype=np.float64) - mean) / (std * 2)
    T, mel = fb.shape
    total = (max(idx) + 1) * target_length
    pad = np.zeros((max(total, T), mel))
    pad[:T] = fb
    return np.stack([pad[i * target_length:(i + 1) * target_length] for i in idx])
