"""What the batched vision front end costs: 640 decoded RGB frames (one training step at batch 64 x 10 frames) to normalised
[640, 3, 224, 224] pixels on the device.

  batch     640 synthetic frames of MIXED sizes around 480 x 640, resident on the host as decoded uint8 arrays.  per_file: the path before
            mico_image_augment - one host-to-device copy and one mico_image_preprocess launch per frame.  batch: ImageProcessor.batch's
            route - pack into one pinned staging buffer, one copy, one table copy, one mico_image_augment launch (`none` table).  Host
            clock from the decoded arrays to a device synchronise, median over --reps; batch_copy_launch leaves the packing out.
  kernels   640 EQUAL 480 x 640 frames resident on the device, plain-resize table: device events around mico_image_preprocess and around
            mico_image_augment, alternating, median over --reps; the worst difference between their outputs; the achieved GB/s of each
            over the region bytes read plus the 12 out_h out_w bytes written per frame; and mico_image_augment with a crop_flip training
            table (random boxes and flips) on the same frames.

    python tools/augment_bench.py [--frames 640] [--reps 15] [--out profiles/augment_bench.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--resolution", type=int, default=224)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--wall-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    from mico_amd import _lib
    from mico_amd.model import transforms as T
    from mico_amd.model.imageprocessor import image_stats
    from mico_amd.model.videoprocessor import augment_packed_device, preprocess_frames_device

    assert torch.cuda.is_available(), "augment_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    n, r = args.frames, args.resolution
    mean, std = image_stats("evaclip01_giant")
    g = torch.Generator().manual_seed(0)
    res = dict(tool="augment_bench", frames=n, resolution=r, reps=args.reps, wall_reps=args.wall_reps)

    def med(v, nd=3):
        return dict(ms=round(statistics.median(v), nd), min_ms=round(min(v), nd), max_ms=round(max(v), nd))

    def wall_ms(fn, reps):
        fn()
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return med(out)

    # ---- 1. a ragged batch from the host ------------------------------------------------------------------------------------------
    hs = torch.randint(400, 561, (n,), generator=g).tolist()
    ws = torch.randint(560, 721, (n,), generator=g).tolist()
    pool = torch.randint(0, 256, (560 * 720 * 3 + n,), dtype=torch.uint8, generator=g)
    frames = [pool[k:k + h * w * 3].view(h, w, 3).clone() for k, (h, w) in enumerate(zip(hs, ws))]
    sizes = list(zip(hs, ws))
    plans = [T.frame_plan(h, w, r, "none", False) for h, w in sizes]

    def per_file():
        return [preprocess_frames_device(f.unsqueeze(0), r, mean, std, dev) for f in frames]

    def pack():
        buf, offs = T.pack_frames(frames, pin=True)
        return buf, [p.row(o, 3 * w) for p, o, (_, w) in zip(plans, offs, sizes)]

    def batch():
        buf, rows = pack()
        return augment_packed_device(buf, rows, sizes, r, mean, std, dev)

    packed, rows = pack()
    a = torch.cat(per_file())
    b = batch()
    res["batch"] = dict(
        source_mb=round(packed.numel() / 1e6, 1),
        per_file=wall_ms(per_file, args.wall_reps),
        batch=wall_ms(batch, args.wall_reps),
        batch_pack_only=wall_ms(pack, args.wall_reps),
        batch_copy_launch=wall_ms(lambda: augment_packed_device(packed, rows, sizes, r, mean, std, dev), args.wall_reps),
        max_abs_diff=float((a - b).abs().max()))
    res["batch"]["per_file_over_batch"] = round(res["batch"]["per_file"]["ms"] / res["batch"]["batch"]["ms"], 2)
    del a, b, packed, frames, pool

    # ---- 2. the kernels alone, equal frames resident on the device ------------------------------------------------------------------
    H, W = 480, 640
    src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    out_old = torch.empty((n, 3, r, r), dtype=torch.float32, device=dev)
    out_new = torch.empty_like(out_old)
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    norm = (mean[0], mean[1], mean[2], 1.0 / std[0], 1.0 / std[1], 1.0 / std[2], stream)

    def table(ps):
        return torch.tensor([p.row(k * H * W * 3, 3 * W) for k, p in enumerate(ps)], dtype=torch.int64).to(dev)

    tab_none = table([T.frame_plan(H, W, r, "none", False)] * n)
    tab_crop = table([T.frame_plan(H, W, r, "crop_flip", True, generator=g) for _ in range(n)])

    def old():
        _lib.check(lib.mico_image_preprocess(src.data_ptr(), n, H, W, out_old.data_ptr(), r, r, *norm), "mico_image_preprocess")

    def new(tab=tab_none):
        _lib.check(lib.mico_image_augment(src.data_ptr(), src.numel(), tab.data_ptr(), n, out_new.data_ptr(), r, r, *norm), "mico_image_augment")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):
        old(), new(), new(tab_crop)
    torch.cuda.synchronize()
    t_old, t_new, t_crop = [], [], []
    for _ in range(args.reps):       # alternating, so drift of the box hits all three alike
        t_old.append(timed(old))
        t_new.append(timed(new))
        t_crop.append(timed(lambda: new(tab_crop)))
    new()
    torch.cuda.synchronize()
    moved = n * (H * W * 3 + 12 * r * r)
    k = dict(frame=[H, W], bytes_moved_mb=round(moved / 1e6, 1), preprocess=med(t_old, 4), augment=med(t_new, 4), augment_crop_flip=med(t_crop, 4),
             max_abs_diff=float((out_old - out_new).abs().max()))
    k["preprocess_gbps"] = round(moved / (k["preprocess"]["ms"] * 1e-3) / 1e9, 1)
    k["augment_gbps"] = round(moved / (k["augment"]["ms"] * 1e-3) / 1e9, 1)
    k["augment_over_preprocess"] = round(k["augment"]["ms"] / k["preprocess"]["ms"], 3)
    res["kernels"] = k
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
