"""Audio front end on the device (mico_kaldi_fbank, mico_resample_sinc, AudioProcessor.fbank / from_waveform / batch / __call__, the
demo's --audio) against tests/audio_oracle.py.  torchaudio is not a dependency, so the filterbank and the resampler are gated against the
fp64 numpy restatement of its published algorithm, with the same restatement in fp32 as the yardstick: the device's worst log-domain
difference to fp64 must stay within 4 x the fp32 restatement's own on the same input (the factor covers another butterfly order and
the device log).  Only the mel resize is pinned to the reference's own call (F.interpolate).  Inputs are seeded; every figure is printed
before it is asserted."""
import functools
import re
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import audio_oracle as A

pytestmark = pytest.mark.gpu

LENGTHS = (400, 1047, 48000)          # one frame; five frames + 7 ignored samples; 298 frames = 74 workgroups and a half-filled one
MELS = (64, 128, 224)


@functools.lru_cache(maxsize=None)
def _signal(n, seed=0):
    """uniform noise of amplitude 0.1 plus a 440 Hz tone of amplitude 0.3 (a pure tone's leakage bins sit at fp32's floor)"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.1, 0.1, n) + 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / 16000.0)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle_fbank(n, mel):
    """(fp64 filterbank, worst |fp32 - fp64|) of _signal(n)"""
    x = _signal(n)
    o64 = A.fbank(x, mel, np.float64)
    o32 = A.fbank(x, mel, np.float32)
    o64.setflags(write=False)
    return o64, float(np.abs(o32.astype(np.float64) - o64).max())


def _proc(mel, resize=None):
    from mico_amd.model.audioprocessor import AudioProcessor
    return AudioProcessor(mel, target_length=100, sample_num=2, resize_melbin_num=resize or mel, training=False)


@pytest.mark.parametrize("mel", MELS)
@pytest.mark.parametrize("n", LENGTHS)
def test_fbank_against_oracle(cuda, n, mel):
    o64, e32 = _oracle_fbank(n, mel)
    fb = _proc(mel).fbank(torch.tensor(_signal(n)))
    assert fb.is_cuda and fb.dtype == torch.float32 and tuple(fb.shape) == o64.shape == (A.num_frames(n), mel)
    got = fb.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - o64).max())
    print(f"[fbank n={n} mel={mel}] device vs fp64 {err:.3e}   fp32 restatement vs fp64 {e32:.3e}   gate {4 * e32:.3e}")
    empty = A.empty_filters(mel)
    floor_cols = {b for b in range(mel) if (got[:, b] == A.LOG_EPS32).all()}
    assert floor_cols == empty                               # empty filters: exactly logf(FLT_EPSILON), and no other column
    assert np.isfinite(got).all()
    assert err <= 4 * e32


@pytest.mark.parametrize("mel", MELS)
def test_fbank_of_silence_is_the_floor(cuda, mel):
    fb = _proc(mel).fbank(torch.zeros(2000))
    assert tuple(fb.shape) == (11, mel)
    assert (fb.cpu().numpy() == A.LOG_EPS32).all()


@pytest.mark.parametrize("mel", [64, 128])
def test_mel_resize_is_f_interpolate(cuda, mel):
    """pinned: the reference's own call (audioprocessor.py:42-43) on the product's unresized rows"""
    x = torch.tensor(_signal(1047))
    plain = _proc(mel).fbank(x).cpu()
    got = _proc(mel, 224).fbank(x).cpu()
    want = F.interpolate(plain[None, None], size=(plain.size(0), 224), mode="bilinear")[0, 0]
    assert tuple(got.shape) == (5, 224)
    tol = 2 * np.spacing(plain.abs().amax(dim=1).numpy().astype(np.float32))
    err = (got - want).abs().amax(dim=1).numpy()
    print(f"[mel resize {mel}->224] worst row error {err.max():.3e}, 2 ulp of the row maximum {tol.min():.3e}")
    assert (err <= tol).all()


def test_packing_and_determinism(cuda):
    p = _proc(64)
    clips = [torch.tensor(_signal(n, seed)) for n, seed in ((400, 1), (1000, 2), (16000, 3))]
    single = [p.fbank(c) for c in clips]
    packed = p.fbank_batch(clips)
    assert [tuple(b.shape) for b in packed] == [(1, 64), (4, 64), (98, 64)]
    for a, b in zip(single, packed):
        assert torch.equal(a, b)                             # a frame's bits depend on its 400 samples alone
    again = p.fbank_batch(clips)
    assert all(torch.equal(a, b) for a, b in zip(packed, again))
    assert torch.equal(p.fbank(clips[2]), single[2])
    # batch() = stacked from_waveform(), a clip below one frame included
    clips.append(torch.tensor(_signal(300, 4)))
    got = p.batch(clips)
    want = torch.stack([p.from_waveform(c) for c in clips])
    assert tuple(got.shape) == (4, 2, 100, 64) and torch.equal(got, want)
    assert not got[3].any()
    # mixed rates: each clip is resampled on its own, then packed
    got = p.batch([clips[1], clips[2]], [22050, 16000])
    assert torch.equal(got[0], p.from_waveform(clips[1], 22050)) and torch.equal(got[1], want[2])


@pytest.mark.parametrize("rate,n", [(44100, 441 * 25 + 1), (48000, 5), (8000, 1000), (22050, 4411)])
def test_resampler_against_oracle(cuda, rate, n):
    """n = 441 * 25 + 1: the ceil in n_out matters; n = 5 at 48 kHz: shorter than the filter's half width; 8 kHz: upsampling"""
    x = np.random.RandomState(rate % 1000 + n).uniform(-1, 1, n).astype(np.float32)
    taps, orig, phases, width = A.resample_taps(rate)
    K = taps.shape[1]
    o64 = A.resample(x, rate, np.float64)
    o32 = A.resample(x, rate, np.float32)
    got = _proc(64).resample(torch.from_numpy(x), rate)
    n_out = -((-phases * n) // orig)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == o64.shape == (n_out,)
    bound = K * 2.0 ** -24 * np.abs(taps).sum(axis=1).max() * float(np.abs(x).max())
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - o64).max())
    print(f"[resample {rate} n={n}] device vs fp64 {err:.3e}   fp32 restatement vs fp64 {np.abs(o32 - o64).max():.3e}   bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(got, _proc(64).resample(torch.from_numpy(x), rate))


def test_resampler_reproduces_a_sine(cuda):
    """not a gate on torchaudio, a sanity check of the algorithm itself: 1 kHz at 44.1 kHz comes out as 1 kHz at 16 kHz"""
    n = 4410
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / 44100.0).astype(np.float32)
    y = _proc(64).resample(torch.from_numpy(x), 44100).cpu().numpy()
    ref = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 16000.0)
    assert len(y) == 1600 and np.abs(y - ref)[200:-200].max() < 1e-3


def test_end_to_end(cuda, tmp_path):
    n, mel = 48000, 64
    p = _proc(mel)
    x = torch.tensor(_signal(n))
    out = p.from_waveform(x)
    fb = p.fbank(x)
    assert tuple(out.shape) == (2, 100, mel) and torch.equal(out, p.from_fbank(fb))
    o64, e32 = _oracle_fbank(n, mel)
    want = A.windows(o64, p.window_indices(o64.shape[0]), 100, p.mean, p.std)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    gate = 4 * e32 / (2 * p.std)
    print(f"[end to end] windows vs fp64 {err:.3e}   gate {gate:.3e}")
    assert err <= gate
    # [c, n]: channel 0 only, host or device input
    assert torch.equal(p.from_waveform(torch.stack([x, -x]).to(cuda)), out)
    # below one frame: zeros of the right shape
    z = p.from_waveform(torch.tensor(_signal(300)))
    assert z.is_cuda and tuple(z.shape) == (2, 100, mel) and not z.any()
    # a 16-bit 22.05 kHz stereo file = from_waveform of the samples it holds
    ints = np.random.RandomState(5).randint(-20000, 20000, size=(22050, 2)).astype("<i2")
    path = str(tmp_path / "clip.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(22050)
        f.writeframes(ints.tobytes())
    samples = torch.from_numpy(ints[:, 0].astype(np.float32) / 32768.0)
    got = p(path)
    assert got is not None and tuple(got.shape) == (2, 100, mel) and torch.equal(got, p.from_waveform(samples, 22050))


def test_demo_audio(cuda, tmp_path, capsys):
    """inference_demo.py --audio: the image's lines are what they are without the flag, then one finite [1, len(texts)] similarity.  (The
    synthetic directory is written here with a 2-block tower, as tests/test_inference_demo_gpu.py does, and passed as --pretrain_dir:
    --synthetic builds the full-depth tower.)"""
    import inference_demo as demo
    from mico_amd import runtime
    from PIL import Image
    rng = np.random.RandomState(0)
    img = str(tmp_path / "test.jpeg")
    Image.fromarray((rng.rand(428, 640, 3) * 255).astype(np.uint8)).save(img, quality=95)
    wav = str(tmp_path / "test.wav")
    with wave.open(wav, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes((_signal(16000) * 32767).astype("<i2").tobytes())
    pdir = str(tmp_path / "MiCo-synth")
    demo.write_synthetic_pretrain_dir(pdir, "evaclip02_base", steps=(3, 12), vision_layers=2, max_vision_sample_num=8)
    texts = ["a man is skiing in a snowy day.", "it's a hot day", "two dogs"]
    old = runtime.compute_dtype()
    try:
        capsys.readouterr()
        demo.main(["--pretrain_dir", pdir, "--image", img, "--texts", *texts])
        base = capsys.readouterr().out
        demo.main(["--pretrain_dir", pdir, "--image", img, "--texts", *texts, "--audio", wav])
        with_audio = capsys.readouterr().out
    finally:
        runtime.set_compute_dtype(old)
    assert with_audio.startswith(base) and len(base.splitlines()) >= 4       # load line, similarity, ITM scores, caption
    extra = with_audio[len(base):].strip()
    assert extra.startswith("tensor([[") and "cuda" in extra
    sim = [float(v) for v in re.findall(r"-?\d+\.\d*(?:e[-+]?\d+)?", extra)]
    assert len(sim) == len(texts) and all(abs(v) <= 1.0 + 1e-3 for v in sim), extra      # a nan or inf prints as no number
