"""Step time of one rank of BASELINE configs[2] (ViT-g/14 image + 4 audio windows + 77 text tokens, b = 64, ITC + ITM + CAP) in training mode
at patch-dropout rates p (FLIP; EVAVisionTransformer.patch_dropout), in bench.py's timed fp16 configuration and staged step
(MiCo.forward(backward_scale=1.0)), forward plus backward.  One model, the rate switched between rounds; the rounds alternate the order of
the rates (A/B/C, C/B/A, ...), each rate is warmed up after every switch, and every timed window is bracketed by device synchronisations.

    python tools/patch_dropout_bench.py [--rates 0,0.5,0.75] [--rounds 4] [--steps 3] [--out profiles/patch_dropout_bench.json]

Prints one JSON line and writes it to --out.  For a kernel profile run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/patch_dropout_bench.py --rates 0.5 --rounds 1 --steps 2 --out <file>`."""
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
    ap.add_argument("--rates", default="0,0.5,0.75")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per rate and round")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps per rate before the first round")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layers", type=int, default=None, help="truncate the tower (default: all 40 blocks)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_dropout_bench.json"))
    args = ap.parse_args()
    rates = [float(r) for r in args.rates.split(",")]

    import bench
    from mico_amd import runtime
    from mico_amd.model import default_cfg
    from mico_amd.model.evaclip import PatchDropout
    from mico_amd.weights import synth_inputs

    dev = torch.device("cuda:0")
    bench.set_precision("fp16")
    torch.manual_seed(0)
    model, _ = bench.build_model(default_cfg("evaclip01_giant", vision_layers=args.layers))
    model.to(dev).train()
    b, task = args.batch, "ret%tva_cap%tva"
    inp = synth_inputs(dict(b=b, vision=1, audio=4, S=77), seed=7)
    batch = {k: v.to(dev) for k, v in inp.items()}
    vis = model.vision_encoder.visual

    def set_rate(p):
        vis.patch_dropout = PatchDropout(p) if p > 0 else torch.nn.Identity()

    def step():
        model.zero_grad(set_to_none=True)
        losses = model(dict(batch), task, compute_loss=True, backward_scale=1.0)
        sum(losses.values()).backward()
        return losses

    times = {p: [] for p in rates}
    peaks, plans, losses = {}, {}, {}
    for p in rates:
        set_rate(p)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(max(1, args.warmup)):
            out = step()
        torch.cuda.synchronize()
        peaks[p] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
        plans[p] = dict(runtime.last_tower_plan or {})
        losses[p] = {k: float(v.detach()) for k, v in out.items()}
        del out
    for r in range(args.rounds):
        for p in (rates if r % 2 == 0 else list(reversed(rates))):
            set_rate(p)
            step()                       # one untimed step after the switch (the plan and the allocator settle on this rate)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            times[p].append((time.perf_counter() - t0) * 1e3 / args.steps)
    base = statistics.median(times[rates[0]])
    res = dict(workload=f"configs[2] one rank: ViT-g/14 image(1) + audio(4) + text(77), b={b}, task {task}, train mode, fp16 timed config, staged step",
               layers=args.layers or 40, device=torch.cuda.get_device_name(dev), rounds=args.rounds, steps_per_window=args.steps,
               rates={str(p): dict(step_ms_median=round(statistics.median(times[p]), 2), step_ms_windows=[round(t, 2) for t in times[p]],
                                   samples_per_s=round(b * 1e3 / statistics.median(times[p]), 2),
                                   ratio_to_first=round(statistics.median(times[p]) / base, 4), peak_allocated_gib=round(peaks[p], 2),
                                   tokens_per_frame=plans[p].get("tokens_per_frame"), frames_per_pass=plans[p].get("frames_per_pass"),
                                   diet=plans[p].get("diet"), losses=losses[p]) for p in rates})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
