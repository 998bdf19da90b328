"""Host side of the audio front end (no GPU): the product's table builders (mico_amd/model/audioprocessor.py, torch fp64) against the
independent numpy restatement in tests/audio_oracle.py, frame bookkeeping, the PCM .wav reader and the C ABI of the two new entry
points.  torchaudio is not a dependency, so nothing is pinned against torchaudio itself: both sides restate its published
algorithm (compliance/kaldi.py fbank, functional.resample) and are compared with each other."""
import ctypes
import os
import re
import wave

import numpy as np
import pytest
import torch

import audio_oracle as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_povey_window_bit_equal():
    from mico_amd.model import audioprocessor as P
    w = P.povey_window()
    assert w.dtype == torch.float32 and w.shape == (400,)
    assert np.array_equal(w.numpy(), A.povey_window(np.float64).astype(np.float32))
    assert w[0] == 0 and w[399] == 0 and abs(float(w[199]) - 1) < 1e-4


@pytest.mark.parametrize("mel", [64, 128, 224])
def test_mel_filter_table(mel):
    from mico_amd.model import audioprocessor as P
    bins, offs, weights = P.mel_filter_table(mel)
    assert bins.dtype == torch.int32 and bins.shape == (mel, 2) and offs.dtype == torch.int32 and weights.dtype == torch.float32
    dense = A.mel_banks(mel, np.float64)
    assert dense.shape == (mel, 257) and not dense[:, 256].any()
    want = A.filter_ranges(dense)
    empty = {b for b in range(mel) if int(bins[b, 1]) == 0}
    assert empty == A.empty_filters(mel)
    assert {64: 0, 128: 1, 224: 16}[mel] == len(empty)
    if mel == 128:
        assert empty == {3}
    total = 0
    for b in range(mel):
        first, count = int(bins[b, 0]), int(bins[b, 1])
        assert int(offs[b]) == total
        if count:
            assert (first, count) == want[b] and first + count <= 256
            assert np.array_equal(weights[total:total + count].numpy(), dense[b, first:first + count].astype(np.float32))
        total += count
    assert weights.numel() == max(total, 1)


@pytest.mark.parametrize("rate,shape", [(44100, (160, 475)), (48000, (1, 41)), (22050, (320, 459)), (8000, (2, 15))])
def test_resample_tap_banks(rate, shape):
    from mico_amd.model import audioprocessor as P
    taps, orig, phases, width = P.resample_taps(rate)
    ref, orig_r, phases_r, width_r = A.resample_taps(rate)
    assert tuple(taps.shape) == shape == ref.shape and taps.dtype == torch.float64
    assert (orig, phases, width) == (orig_r, phases_r, width_r) and shape[1] == 2 * width + orig
    assert np.abs(taps.numpy() - ref).max() <= 1e-12


@pytest.mark.parametrize("mel", [64, 128])
def test_oracle_mel_resize_is_f_interpolate(mel):
    """the restatement's resize formula against the reference's own call (audioprocessor.py:42-43), both in fp64"""
    fb = torch.randn(7, mel, dtype=torch.float64, generator=torch.Generator().manual_seed(mel)) * 10
    want = torch.nn.functional.interpolate(fb[None, None], size=(7, 224), mode="bilinear")[0, 0]
    assert np.abs(A.mel_resize(fb.numpy(), 224) - want.numpy()).max() < 1e-12
    assert A.mel_resize(fb.numpy(), mel) is not None and np.array_equal(A.mel_resize(fb.numpy(), mel), fb.numpy())


def test_frame_count_and_starts():
    from mico_amd.model import audioprocessor as P
    assert [P.num_frames(n) for n in (0, 399, 400, 559, 560, 1047, 48000)] == [0, 0, 1, 1, 2, 5, 298]
    assert [A.num_frames(n) for n in (0, 399, 400, 559, 560, 1047, 48000)] == [0, 0, 1, 1, 2, 5, 298]
    lengths = [400, 399, 1000, 560, 16000]
    starts, counts = P.frame_start_table(lengths)
    ref, counts_r = A.frame_starts(lengths)
    assert starts.dtype == torch.int64 and counts == counts_r == [1, 0, 4, 2, 98]
    assert np.array_equal(starts.numpy(), ref)
    assert starts[:6].tolist() == [0, 799, 959, 1119, 1279, 1799]
    # every frame lies inside its clip
    base = 0
    it = iter(starts.tolist())
    for n, t in zip(lengths, counts):
        for _ in range(t):
            s = next(it)
            assert base <= s and s + 400 <= base + n
        base += n
    empty, c0 = P.frame_start_table([])
    assert empty.numel() == 0 and c0 == []


def _write_wav(path, ints, width, channels, rate):
    """ints [n, channels]: 8-bit values are unsigned, the others signed little-endian"""
    if width == 1:
        raw = ints.astype(np.uint8).tobytes()
    elif width == 3:
        u = ints.astype(np.int64) & 0xFFFFFF
        raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8).tobytes()
    else:
        raw = ints.astype({2: "<i2", 4: "<i4"}[width]).tobytes()
    with wave.open(path, "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_wav_reader(tmp_path, width, channels):
    from mico_amd.model import audioprocessor as P
    rng = np.random.RandomState(10 * width + channels)
    bits = 8 * width
    lo, hi = (0, 256) if width == 1 else (-(1 << (bits - 1)), 1 << (bits - 1))
    ints = rng.randint(lo, hi, size=(37, channels), dtype=np.int64)
    ints[0, 0], ints[1, 0] = lo, hi - 1                      # both ends of the range
    path = str(tmp_path / f"pcm{bits}_{channels}.wav")
    _write_wav(path, ints, width, channels, 22050)
    got, rate = P.read_wav(path)
    assert rate == 22050 and got.dtype == torch.float32 and tuple(got.shape) == (channels, 37)
    want = ((ints - 128) / 128.0 if width == 1 else ints / float(1 << (bits - 1))).astype(np.float32)
    assert np.array_equal(got.numpy(), want.T)               # channel 0 first
    assert float(got.min()) == -1.0 and float(got.max()) <= 1.0      # (2^31 - 1) / 2^31 rounds to 1.0 in fp32


def test_other_container_needs_torchaudio(tmp_path, capsys):
    from mico_amd.model.audioprocessor import AudioProcessor
    try:
        import torchaudio  # noqa: F401
        pytest.skip("torchaudio is installed")
    except ImportError:
        pass
    p = AudioProcessor(64, 224, 2, device="cpu")
    f = str(tmp_path / "a.flac")
    open(f, "wb").write(b"fLaC")
    with pytest.raises(ImportError, match="flac"):
        p(f)
    # the reference's own behaviour is kept: a missing file gives zeros ...
    z = p(str(tmp_path / "missing.wav"))
    assert tuple(z.shape) == (2, 224, 64) and not z.any()
    # ... and an undecodable file a print and None
    bad = str(tmp_path / "bad.wav")
    open(bad, "w").write("x")
    assert p(bad) is None and capsys.readouterr().out.strip()


def _layout(fn):
    n = fn(None, 0)
    buf = (ctypes.c_int * n)()
    assert fn(buf, n) == n
    return list(buf)


def test_abi_symbols_struct_and_version():
    """mico_fbank_params has its own layout table (mico_fbank_params_layout, same format as mico_struct_layout): size and every field
    offset of the ctypes mirror, and the header's field list in declaration order."""
    from mico_amd import _lib
    l = _lib.lib()
    for s in ("mico_kaldi_fbank", "mico_resample_sinc", "mico_fbank_params_layout"):
        assert hasattr(l, s) and s in _lib.PROTOTYPES
    assert l.mico_version() == _lib.ABI_VERSION >= 121
    size, *offs = _layout(l.mico_fbank_params_layout)
    assert offs[-1] == -1
    offs = offs[:-1]
    cls = _lib.FbankParams
    assert ctypes.sizeof(cls) == size
    assert [getattr(cls, n).offset for n, _ in cls._fields_] == offs
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mico_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct mico_fbank_params \{(.*?)\} mico_fbank_params;", hdr, re.S).group(1)
    names = [re.findall(r"([A-Za-z_][A-Za-z0-9_]*)$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in cls._fields_]
    assert len(_layout(l.mico_struct_layout)) > 0          # the four older structs keep their table


def test_bad_arguments_are_errors_not_launches():
    """MICO_CHECK paths run on the host before any launch"""
    from mico_amd import _lib
    l = _lib.lib()
    assert l.mico_kaldi_fbank(None, None) == -22
    p = _lib.FbankParams(wave=8, n_samples=400, T=1, scale=1.0, window=8, twiddle=8, mel=300, mel_out=300, filt_bins=8, filt_off=8, filt_w=8,
                         out=8)
    assert l.mico_kaldi_fbank(ctypes.byref(p), None) == -22 and b"mel" in l.mico_last_error_string()
    p.mel = p.mel_out = 64
    p.T = 2                                                  # two frames do not fit 400 samples
    assert l.mico_kaldi_fbank(ctypes.byref(p), None) == -22
    assert l.mico_resample_sinc(16, 10, 16, 40, 44, 3, 1, 19, 16, 4, None) == -22        # K != 2 width + orig
    assert l.mico_resample_sinc(16, 10, 16, 41, 41, 3, 1, 19, 16, 4, None) == -22        # ldt not a multiple of 4
    assert l.mico_resample_sinc(16, 10, 16, 41, 44, 3, 1, 19, 16, 3, None) == -22        # n_out != ceil(10 / 3)
    # 44101 Hz shares no factor with 16000: the span of one workgroup cannot be staged
    assert l.mico_resample_sinc(16, 10, 16, 2 * 268 + 44101, 2 * 268 + 44101 + 3, 44101, 16000, 268, 16, 4, None) == -22
    assert b"LDS" in l.mico_last_error_string()
