"""What the device-side audio front end costs: 64 clips of 10 s to log-mel filterbanks (224 filters), clips packed into one
mico_kaldi_fbank launch, once from 16 kHz and once from 44.1 kHz (64 mico_resample_sinc launches first).

  device    device events around the launches on resident waveforms, median over --reps: the filterbank launch alone, the resampler
            launches alone (44.1 kHz run), and the whole AudioProcessor.batch (resample + filterbank + the per-clip window kernel;
            host clock to a device synchronise, so it includes the host's table building and launch overhead)
  host      the same batch through a plain fp32 torch restatement of torchaudio's algorithm on the CPU (conv1d resampler, unfold + rfft +
            matmul filterbank) at --threads threads (16), median over --host-reps
  floor     the bytes the filterbank launch has to move at 16 kHz - every sample is read once per frame it falls in (400 / 160 = 2.5
            times), the log-mel rows are written once - and the time they take at the HBM rate given by --hbm-tbps

    python tools/fbank_bench.py [--clips 64] [--seconds 10] [--reps 15] [--out profiles/fbank_bench.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def host_resample(x, rate):
    """torchaudio.functional.resample(x, rate, 16000) restated in fp32 torch: [B, n] -> [B, ceil(n 16000 / rate)]"""
    g = math.gcd(rate, 16000)
    orig, new = rate // g, 16000 // g
    base = min(orig, new) * 0.99
    width = math.ceil(6 * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = (torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx) * base
    t = t.clamp(-6, 6)
    window = torch.cos(t * math.pi / 12) ** 2
    t = t * math.pi
    kernel = (torch.where(t == 0, torch.ones_like(t), t.sin() / torch.where(t == 0, torch.ones_like(t), t)) * window * (base / orig)).float()
    n = x.shape[-1]
    y = F.conv1d(F.pad(x[:, None], (width, width + orig)), kernel, stride=orig)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :-((-new * n) // orig)]


def host_fbank(x, mel):
    """kaldi.fbank(x * 2**15, num_mel_bins=mel, 16 kHz, 25 ms / 10 ms) restated in fp32 torch, per clip of the batch [B, n] -> [B, T, mel]"""
    fr = (x * 32768.0).unfold(1, 400, 160)
    fr = fr - fr.mean(dim=2, keepdim=True)
    fr = fr - 0.97 * torch.cat((fr[..., :1], fr[..., :-1]), dim=2)
    fr = fr * torch.hann_window(400, periodic=False).pow(0.85)
    spec = torch.fft.rfft(F.pad(fr, (0, 112)), dim=2)
    power = spec.real ** 2 + spec.imag ** 2

    def mel_of(f):
        return 1127.0 * torch.log(1.0 + f / 700.0)
    lo, hi = mel_of(torch.tensor(20.0)), mel_of(torch.tensor(8000.0))
    d = (hi - lo) / (mel + 1)
    left = lo + torch.arange(mel)[:, None] * d
    m_k = mel_of(31.25 * torch.arange(256))[None]
    w = torch.minimum((m_k - left) / d, (left + 2 * d - m_k) / d).clamp_min(0)
    return torch.clamp_min(power[..., :256] @ w.T, 1.1920929e-07).log()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--mel", type=int, default=224)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--hbm-tbps", type=float, default=8.0, help="HBM rate the byte floor is quoted at (MI355X data sheet: 8 TB/s)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_bench.json"))
    args = ap.parse_args()
    from mico_amd.model.audioprocessor import AudioProcessor, frame_start_table

    assert torch.cuda.is_available(), "fbank_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    proc = AudioProcessor(args.mel, 224, 4, resize_melbin_num=args.mel, training=False, device=dev)
    res = dict(tool="fbank_bench", clips=args.clips, seconds=args.seconds, mel=args.mel, reps=args.reps, host_threads=args.threads)

    def device_ms(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return dict(ms=round(statistics.median(out), 4), min_ms=round(min(out), 4), max_ms=round(max(out), 4))

    def wall_ms(fn, reps, sync):
        out = []
        for _ in range(reps):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if sync:
                torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return dict(ms=round(statistics.median(out), 3), min_ms=round(min(out), 3), max_ms=round(max(out), 3))

    for rate in (16000, 44100):
        n = int(round(args.seconds * rate))
        host = torch.rand((args.clips, n), generator=torch.Generator().manual_seed(rate)) * 0.2 - 0.1
        clips = list(host.to(dev))
        r = dict(samples_per_clip=n)
        if rate != 16000:
            r["resample_launches"] = device_ms(lambda: [proc.resample(c, rate) for c in clips], args.reps)
        at16 = [proc.resample(c, rate) for c in clips]
        starts, counts = frame_start_table([c.numel() for c in at16])
        packed, starts = torch.cat(at16), starts.to(dev)
        r["frames"] = int(starts.numel())
        r["fbank_launch"] = device_ms(lambda: proc._fbank_launch(packed, starts, starts.numel()), args.reps)
        r["batch_wall"] = wall_ms(lambda: proc.batch(clips, rate), args.reps, True)
        if rate == 16000:
            rd, wr = 4.0 * 400 * starts.numel(), 4.0 * args.mel * starts.numel()
            r["byte_floor"] = dict(read_mb=round(rd / 1e6, 1), write_mb=round(wr / 1e6, 1), hbm_tbps=args.hbm_tbps,
                                   us=round((rd + wr) / (args.hbm_tbps * 1e12) * 1e6, 1))
            r["fbank_launch_over_floor"] = round(r["fbank_launch"]["ms"] * 1e3 / r["byte_floor"]["us"], 1)

        def on_host():
            x = host if rate == 16000 else host_resample(host, rate)
            return host_fbank(x, args.mel)
        on_host()
        r["host_torch_fp32"] = wall_ms(on_host, args.host_reps, False)
        r["host_over_device_batch"] = round(r["host_torch_fp32"]["ms"] / r["batch_wall"]["ms"], 1)
        # the two routes agree (noise input: no bin at fp32's floor)
        fb_dev = proc._fbank_launch(packed, starts, starts.numel()).cpu()
        r["max_abs_diff_device_vs_host"] = round(float((fb_dev - on_host().reshape(-1, args.mel)).abs().max()), 6)
        res[f"from_{rate}"] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
