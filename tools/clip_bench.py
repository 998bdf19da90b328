"""What global-norm gradient clipping costs in the optimizer step, on the parameter set bench.py trains (MiCo with the ViT-g/14 towers:
~1.19 B parameters, 4.75 GB of fp32 gradients; shapes from a build on the meta device, seeded random values and gradients, no forward pass):

  kernels   mico_grad_sumsq (sum of squares + overflow flag) against mico_grads_finite (overflow flag only) on the SAME descriptor table - the
            same bytes read once each.  Device events around the launch, median over --reps alternating runs; GB/s = gradient bytes / time.
            Acceptance: the new kernel reaches >= 0.9x the bandwidth of mico_grads_finite.
  steps     one GradScaler.step(optimizer) in three forms, host clock around work that ends in a device synchronise, median over --reps
            alternating rounds:
              unclipped   mico_grads_finite + mico_adamw_step (the path of an optimizer without max_grad_norm)
              clipped     mico_grad_sumsq + mico_grad_clip_coef + mico_adamw_step_dev (optimizer.max_grad_norm set)
              torch_clip  torch.nn.utils.clip_grad_norm_(parameters, max_norm) and then the unclipped form
            (The times do not depend on the gradient values; torch_clip rescales the gradients in place, the other forms leave them alone.)

    python tools/clip_bench.py [--vision evaclip01_giant] [--layers N] [--reps 15] [--max_norm 1.0] [--out profiles/clip_bench.json]

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

NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vision", default="evaclip01_giant")
    ap.add_argument("--layers", type=int, default=None, help="truncate the towers (rehearsal only)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--max_norm", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    from mico_amd import _lib, optim
    from mico_amd.model import MiCo, default_cfg

    assert torch.cuda.is_available(), "clip_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        shapes = [(n, tuple(p.shape)) for n, p in MiCo(default_cfg(args.vision, vision_layers=args.layers)).named_parameters()]
    gen = torch.Generator(device=dev).manual_seed(0)
    params, decay, nodecay = [], [], []
    for n, s in shapes:
        p = torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02)
        p.grad = torch.randn(s, device=dev, generator=gen) * 1e-3
        params.append(p)
        (nodecay if any(k in n for k in NO_DECAY) else decay).append(p)
    opt = optim.AdamW([dict(params=decay, weight_decay=0.01, lr=1e-6), dict(params=nodecay, weight_decay=0.0, lr=1e-6)], lr=1e-6,
                      betas=(0.9, 0.98))
    numel = sum(p.numel() for p in params)
    gbytes = 4.0 * numel / 1e9
    res = dict(tool="clip_bench", vision=args.vision, layers=args.layers, tensors=len(params), parameters=numel, grad_gb=round(gbytes, 3),
               reps=args.reps, max_norm=args.max_norm)

    # ---- the two read-only kernels on one table ----
    lib = _lib.lib()
    grads = opt._grads()
    table, (ct, cs, n) = optim._grad_table(grads, opt._chunk_cache)
    sumsq = torch.empty(n, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    head = (table.data_ptr(), len(grads), ct.data_ptr(), cs.data_ptr(), n, optim.CHUNK)
    kernels = {
        "mico_grads_finite": lambda: _lib.check(lib.mico_grads_finite(*head, flag.data_ptr(), stream), "mico_grads_finite"),
        "mico_grad_sumsq": lambda: _lib.check(lib.mico_grad_sumsq(*head, 1.0, sumsq.data_ptr(), flag.data_ptr(), stream), "mico_grad_sumsq"),
    }
    ktimes = {k: [] for k in kernels}
    for k in kernels:                                  # warm-up: code objects loaded, the table resident
        for _ in range(3):
            kernels[k]()
    torch.cuda.synchronize()
    for r in range(args.reps):
        for k in (list(kernels) if r % 2 == 0 else list(kernels)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kernels[k]()
            e1.record()
            e1.synchronize()
            ktimes[k].append(e0.elapsed_time(e1))
    assert flag.item() == 0.0
    for k in kernels:
        ms = statistics.median(ktimes[k])
        res[k] = dict(ms=round(ms, 4), gb_per_s=round(gbytes / (ms * 1e-3), 1), min_ms=round(min(ktimes[k]), 4), max_ms=round(max(ktimes[k]), 4))
    res["sumsq_over_finite_bandwidth"] = round(res["mico_grad_sumsq"]["gb_per_s"] / res["mico_grads_finite"]["gb_per_s"], 3)
    res["chunks"] = n
    del grads, table, sumsq

    # ---- the scaler step in three forms ----
    sc = optim.GradScaler(init_scale=1.0)

    def unclipped():
        opt.max_grad_norm = None
        sc.step(opt)
        sc.update()

    def clipped():
        opt.max_grad_norm = args.max_norm
        sc.step(opt)
        sc.update()

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(params, args.max_norm)
        unclipped()

    forms = {"unclipped": unclipped, "clipped": clipped, "torch_clip": torch_clip}
    names = list(forms)
    stimes = {f: [] for f in names}
    for f in names:                                    # warm-up: optimizer state allocated, every kernel loaded
        for _ in range(2):
            forms[f]()
    torch.cuda.synchronize()
    for r in range(args.reps):
        for f in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            forms[f]()
            torch.cuda.synchronize()
            stimes[f].append((time.perf_counter() - t0) * 1e3)
    for f in names:
        res["step_" + f] = dict(ms=round(statistics.median(stimes[f]), 3), min_ms=round(min(stimes[f]), 3), max_ms=round(max(stimes[f]), 3))
    res["clipped_over_unclipped"] = round(res["step_clipped"]["ms"] / res["step_unclipped"]["ms"], 4)
    res["last_grad_norm"] = float(opt.last_grad_norm)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
