"""Audio preprocessing with the reference's surface (model/audioprocessor.py:15-83), from a waveform to the tower's windows on the device:
resample to 16 kHz (mico_resample_sinc), Kaldi log-mel filterbank with the optional mel resize (mico_kaldi_fbank), then normalise by
(mean, 2 std), zero-pad to whole windows, cut into target_length windows and pick sample_num of them (mico_fbank_windows).  The
reference takes the first two steps from torchaudio, which is not a dependency here; instead they are restated from torchaudio's published
algorithms, every table computed on the host in double precision.  PCM .wav files are decoded with the standard library; any other
container still needs torchaudio, for decoding only."""
import ctypes
import math
import os

import numpy as np
import torch

from .. import _lib
from .videoprocessor import sample_indices, split  # noqa: F401  (same helper as audioprocessor.py:8-12)

SAMPLE_RATE = 16000
FRAME_LENGTH, FRAME_SHIFT, NFFT = 400, 160, 512     # 25 ms / 10 ms at 16 kHz, padded to the next power of two


def num_frames(n):
    """Kaldi snip_edges: only frames that lie inside the clip."""
    return 1 + (n - FRAME_LENGTH) // FRAME_SHIFT if n >= FRAME_LENGTH else 0


def frame_start_table(lengths):
    """First sample of every frame of clips packed back to back -> (int64 tensor [sum T], [T per clip])."""
    starts, counts, base = [], [], 0
    for n in lengths:
        t = num_frames(int(n))
        starts.append(base + FRAME_SHIFT * torch.arange(t, dtype=torch.int64))
        counts.append(t)
        base += int(n)
    return (torch.cat(starts) if starts else torch.zeros(0, dtype=torch.int64)), counts


def povey_window():
    """(0.5 - 0.5 cos(2 pi j / 399)) ** 0.85 in fp64, rounded once -> fp32 [400]"""
    return torch.tensor([(0.5 - 0.5 * math.cos(2.0 * math.pi * j / (FRAME_LENGTH - 1))) ** 0.85 for j in range(FRAME_LENGTH)],
                        dtype=torch.float64).to(torch.float32)


def fft_twiddles():
    """(cos, -sin)(2 pi m / 512), m < 512, in fp64, rounded once -> fp32 [512, 2]"""
    a = 2.0 * math.pi * torch.arange(NFFT, dtype=torch.float64) / NFFT
    return torch.stack((torch.cos(a), -torch.sin(a)), dim=1).to(torch.float32).contiguous()


def mel_filter_table(mel):
    """The `mel` triangular Kaldi filters between 20 Hz and 8 kHz on FFT bins 0..255 -> (bins int32 [mel, 2] = (first bin, count),
    offsets int32 [mel] into the packed weights, weights fp32), computed in fp64.  A filter narrower than the bin spacing can miss every
    bin: count 0."""
    def mel_of(f):
        return 1127.0 * torch.log(1.0 + f / 700.0)
    lo, hi = (mel_of(torch.tensor(f, dtype=torch.float64)) for f in (20.0, 8000.0))
    d = (hi - lo) / (mel + 1)
    m_k = mel_of(torch.arange(NFFT // 2, dtype=torch.float64) * (SAMPLE_RATE / NFFT))
    bins, offs, weights = [], [], []
    total = 0
    for b in range(mel):
        left = lo + b * d
        centre, right = left + d, left + 2.0 * d
        w = torch.minimum((m_k - left) / (centre - left), (right - m_k) / (right - centre)).clamp_min(0.0)
        nz = torch.nonzero(w).flatten()
        first, count = (int(nz[0]), int(nz[-1] - nz[0]) + 1) if nz.numel() else (0, 0)
        bins.append((first, count))
        offs.append(total)
        weights.append(w[first:first + count])
        total += count
    return (torch.tensor(bins, dtype=torch.int32), torch.tensor(offs, dtype=torch.int32),
            torch.cat(weights).to(torch.float32) if total else torch.zeros(1, dtype=torch.float32))


def resample_taps(rate, new_rate=SAMPLE_RATE):
    """The tap bank of torchaudio.transforms.Resample(rate, new_rate) (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) in fp64
    -> (taps [P, K], orig, P, width): out[f P + p] = sum_j taps[p, j] x[f orig + j - width]."""
    g = math.gcd(int(rate), int(new_rate))
    orig, P = int(rate) // g, int(new_rate) // g
    base = min(orig, P) * 0.99
    width = math.ceil(6 * orig / base)
    j = torch.arange(-width, width + orig, dtype=torch.float64)
    p = torch.arange(P, dtype=torch.float64)
    t = ((-p / P)[:, None] + (j / orig)[None, :]) * base
    t = t.clamp(-6.0, 6.0)
    window = torch.cos(t * math.pi / 12.0) ** 2
    t = t * math.pi
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / torch.where(t == 0, torch.ones_like(t), t))
    return sinc * window * (base / orig), orig, P, width


def read_wav(path):
    """PCM .wav -> (float32 [channels, n] in [-1, 1), rate), scaled as torchaudio.load does: 8-bit unsigned (v - 128) / 128, 16 / 24 / 32-bit
    signed v / 2^(bits - 1)."""
    import wave
    with wave.open(path, "rb") as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if f.getcomptype() != "NONE":
            raise ValueError(f"{path}: compressed wav ({f.getcomptype()}) is not supported")
        raw = f.readframes(n)
    if width == 1:
        v = (np.frombuffer(raw, dtype=np.uint8).astype(np.float64) - 128.0) / 128.0
    elif width == 2:
        v = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) - ((b[:, 2] & 0x80) << 17)).astype(np.float64) / 8388608.0
    elif width == 4:
        v = np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples are not supported")
    return torch.from_numpy(v.astype(np.float32).reshape(-1, ch).T.copy()), rate


class AudioProcessor(object):
    def __init__(self, melbins, target_length, sample_num, frame_shift=10, resize_melbin_num=224, mean=15.41663, std=6.55582,
                 training=True, device="cuda"):
        self.melbins = melbins
        self.target_length = target_length
        self.training = training
        self.frame_shift = frame_shift
        self.sample_num = sample_num
        self.resize_melbin_num = resize_melbin_num
        self.mean = mean
        self.std = std
        self.device = device
        self._fbank_tables = {}    # melbins -> device tables of mico_kaldi_fbank
        self._tap_banks = {}       # source rate -> device tap bank of mico_resample_sinc

    def window_indices(self, src_length):
        """audioprocessor.py:50-62: number of target_length windows after padding, split into sample_num groups, one pick each."""
        pad_len = max(self.target_length * self.sample_num - src_length, self.target_length - src_length % self.target_length)
        total = (src_length + pad_len) // self.target_length
        return sample_indices(split(list(range(total)), self.sample_num), self.training)

    def from_fbank(self, fbank):
        """fbank [T, mel] (already resize_melbin_num wide) -> [sample_num, target_length, mel] on the device."""
        fb = fbank.to(self.device, torch.float32).contiguous()
        T, mel = fb.shape
        idx = torch.tensor(self.window_indices(T), dtype=torch.int32, device=fb.device)
        out = torch.empty((idx.numel(), self.target_length, mel), dtype=torch.float32, device=fb.device)
        rc = _lib.lib().mico_fbank_windows(fb.data_ptr(), T, mel, idx.data_ptr(), idx.numel(), self.target_length, float(self.mean),
                                           1.0 / (float(self.std) * 2), out.data_ptr(), torch.cuda.current_stream(fb.device).cuda_stream)
        _lib.check(rc, "mico_fbank_windows")
        return out

    # ---- waveform -> filterbank on the device ----
    def _tables(self):
        t = self._fbank_tables.get(self.melbins)
        if t is None:
            bins, offs, weights = mel_filter_table(self.melbins)
            t = tuple(x.to(self.device) for x in (povey_window(), fft_twiddles(), bins, offs, weights))
            self._fbank_tables[self.melbins] = t
        return t

    def _taps(self, rate):
        t = self._tap_banks.get(rate)
        if t is None:
            taps, orig, P, width = resample_taps(rate)
            K = taps.shape[1]
            ldt = (K + 3) // 4 * 4        # 16-byte rows, zeros past K
            padded = torch.zeros((P, ldt), dtype=torch.float32)
            padded[:, :K] = taps.to(torch.float32)
            t = (padded.to(self.device), K, ldt, orig, P, width)
            self._tap_banks[rate] = t
        return t

    def _mono(self, wave):
        """[n] or [c, n] -> channel 0 as a contiguous fp32 device vector (kaldi.fbank reads channel 0 only)"""
        wave = torch.as_tensor(wave)
        if wave.dim() == 2:
            wave = wave[0]
        if wave.dim() != 1:
            raise ValueError(f"waveform must be [n] or [channels, n], got {tuple(wave.shape)}")
        return wave.to(self.device, torch.float32).contiguous()

    def resample(self, wave, rate):
        """[n] at `rate` -> [ceil(n 16000 / rate)] at 16 kHz on the device (torchaudio.transforms.Resample(rate, 16000))."""
        x = self._mono(wave)
        if int(rate) == SAMPLE_RATE:
            return x
        taps, K, ldt, orig, P, width = self._taps(int(rate))
        n = x.numel()
        n_out = -((-P * n) // orig)
        out = torch.empty(n_out, dtype=torch.float32, device=x.device)
        rc = _lib.lib().mico_resample_sinc(x.data_ptr(), n, taps.data_ptr(), K, ldt, orig, P, width, out.data_ptr(), n_out,
                                           torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(rc, "mico_resample_sinc")
        return out

    def _fbank_launch(self, wave, frame_start, T):
        """wave: fp32 device vector (clips back to back); frame_start: int64 device [T] or None -> [T, resize_melbin_num]"""
        out = torch.empty((T, self.resize_melbin_num), dtype=torch.float32, device=wave.device)
        if T == 0:
            return out
        window, twiddle, bins, offs, weights = self._tables()
        p = _lib.FbankParams(wave=wave.data_ptr(), n_samples=wave.numel(), frame_start=frame_start.data_ptr() if frame_start is not None else None,
                             T=T, scale=32768.0, window=window.data_ptr(), twiddle=twiddle.data_ptr(), mel=self.melbins,
                             mel_out=self.resize_melbin_num, filt_bins=bins.data_ptr(), filt_off=offs.data_ptr(), filt_w=weights.data_ptr(),
                             out=out.data_ptr())
        rc = _lib.lib().mico_kaldi_fbank(ctypes.byref(p), torch.cuda.current_stream(wave.device).cuda_stream)
        _lib.check(rc, "mico_kaldi_fbank")
        return out

    def fbank(self, wave, rate=SAMPLE_RATE):
        """wave [n] or [c, n] float in [-1, 1] (host or device) at `rate` -> Kaldi log-mel filterbank [T, resize_melbin_num] on the device:
        kaldi.fbank(wave * 2**15, num_mel_bins=melbins, sample_frequency=16000, frame_length=25, frame_shift=10) of the clip resampled to
        16 kHz, resized along the mel axis when resize_melbin_num != melbins (audioprocessor.py:34-43)."""
        x = self.resample(wave, rate)
        return self._fbank_launch(x, None, num_frames(x.numel()))

    def _zero_windows(self):
        return torch.zeros((self.sample_num, self.target_length, self.resize_melbin_num), dtype=torch.float32, device=self.device)

    def from_waveform(self, wave, rate=SAMPLE_RATE):
        """-> [sample_num, target_length, mel].  A clip shorter than one frame has an empty filterbank: all-zero windows (what the reference's
        pad-then-slice yields, audioprocessor.py:46-52), no launch."""
        fb = self.fbank(wave, rate)
        return self.from_fbank(fb) if fb.shape[0] else self._zero_windows()

    def fbank_batch(self, waves, rates=None):
        """-> one [T_i, resize_melbin_num] row block per clip, all from ONE mico_kaldi_fbank launch over the clips packed back to back (a
        host-built frame_start table: one H2D copy, no device sync).  rates: one per clip, one for all, or None for 16 kHz."""
        rates = [SAMPLE_RATE] * len(waves) if rates is None else ([rates] * len(waves) if isinstance(rates, int) else list(rates))
        clips = [self.resample(w, r) for w, r in zip(waves, rates)]
        starts, counts = frame_start_table([c.numel() for c in clips])
        packed = torch.cat(clips) if clips else torch.zeros(0, dtype=torch.float32, device=self.device)
        fb = self._fbank_launch(packed, starts.to(packed.device, non_blocking=True), int(starts.numel()))
        return list(fb.split(counts)) if counts else []

    def batch(self, waves, rates=None):
        """-> [B, sample_num, target_length, mel]: fbank_batch, then the window kernel per clip on its row block."""
        out = [self.from_fbank(fb) if fb.shape[0] else self._zero_windows() for fb in self.fbank_batch(waves, rates)]
        return torch.stack(out) if out else torch.zeros((0, self.sample_num, self.target_length, self.resize_melbin_num), device=self.device)

    def load(self, wav_file):
        """-> (float32 [channels, n], rate): PCM .wav through the standard library, anything else through torchaudio (decoding only)."""
        ext = os.path.splitext(wav_file)[1].lower()
        if ext in (".wav", ".wave"):
            return read_wav(wav_file)
        try:
            import torchaudio
        except ImportError as e:
            raise ImportError(f"AudioProcessor.__call__ needs torchaudio to decode {ext or 'this'} files (only PCM .wav is read without "
                              "it); pass samples to from_waveform() or a filterbank to from_fbank() instead") from e
        return torchaudio.load(wav_file)

    def __call__(self, wav_file):
        if not os.path.exists(wav_file):
            print("not have audios", wav_file)
            return torch.zeros(self.sample_num, self.target_length, self.melbins)
        try:
            wave, rate = self.load(wav_file)
            return self.from_waveform(wave, rate)
        except ImportError:      # no decoder for this container: an error, as before
            raise
        except Exception as e:   # audioprocessor.py:74-76
            print(e)
            return
