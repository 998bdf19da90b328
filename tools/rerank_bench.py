"""ITM re-ranking time of a retrieval evaluation, three forms of the same scores, BERT only (synthetic weights; the features and the
condition tokens come from the seeded generator - no tower runs).  g/14-shaped `tva`: Nq = Nc = 1000, E = 1285 condition tokens per
candidate, k = 50 in both directions, 77-token texts with attended lengths drawn like caption lengths (8 .. 40 tokens), plain fp16.
    a  per-pair:  encoder_hidden_states expanded per pair - every pair projects its candidate's tokens to K/V in all 12 layers
    b  indexed, trim_text=False: every candidate projected once, its pairs read the K/V memory by index (mico_attn_params.kv_index)
    c  indexed, trim_text=True:  as b, token rows cut to the longest attended length of the sub-batch
All three walk the same candidate-major pair list (evaluation.plan_pairs) in sub-batches of --pair-batch pairs.  After one warm-up of every
form the rounds alternate their order; every timed window is bracketed by device synchronisations.

    python tools/rerank_bench.py [--nq 1000 --nc 1000 --k 50 --rounds 2] [--forms a,b,c] [--out profiles/rerank_bench.json]
    python tools/rerank_bench.py --gpu-steps           # each GPU step in a child process under its own timeout, first failure ends the run:
                                                       # the bench, `rocprofv3 --kernel-trace --stats` of forms a and c -> profiles/rerank_kernels.txt,
                                                       # `rocprofv3 --pmc FETCH_SIZE` of tools/probes/kv_index_locality.py -> profiles/rerank_kv_locality.json

Prints one JSON line (seconds per form, the ratios a/b and a/c, the shape-derived counts) and writes it to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, D, I, H = 12, 768, 3072, 12


def shape_counts(pairs, cands, E, S, S_trim_rows, nq, nc, k):
    """Counts derived from the shapes alone (nothing measured).  Per pair and layer the text side is the self-attention block, the
    cross-attention query / output projections and the FFN over S rows; the K/V projection of a candidate is E rows x [D -> 2 D] per layer."""
    kv_proj_flop = 2 * E * D * 2 * D * L                        # one candidate, all layers
    kv_bytes = E * L * 2 * D * 2                                # its K/V memory, 16-bit
    text_lin = 2 * D * (3 * D + D + D + D + 2 * I) * L         # per token row: qkv, self-out, cross q, cross-out, FFN
    attn = lambda s: (4 * s * s * D + 4 * s * E * D) * L        # QK^T + PV, self and cross
    text_flop = lambda rows, s: rows * text_lin + (rows / s) * attn(s) if s else 0
    d = dict(pairs=pairs, candidates_with_pairs=cands, E=E, S=S, k=k, nq=nq, nc=nc,
             kv_bytes_per_candidate=kv_bytes, kv_proj_flop_per_candidate=kv_proj_flop,
             a=dict(kv_projections=pairs, kv_proj_flop=pairs * kv_proj_flop, kv_bytes_materialised=pairs * kv_bytes,
                    text_flop=text_flop(pairs * S, S)),
             b=dict(kv_projections=cands, kv_proj_flop=cands * kv_proj_flop, kv_bytes_materialised=cands * kv_bytes,
                    text_flop=text_flop(pairs * S, S)),
             c=dict(kv_projections=cands, kv_proj_flop=cands * kv_proj_flop, kv_bytes_materialised=cands * kv_bytes,
                    text_rows=S_trim_rows, text_flop=S_trim_rows * text_lin + pairs * attn(S_trim_rows / max(pairs, 1))))
    # cross-attention K/V reads: algorithmic = every distinct (candidate, head) block once per layer; per pair = what a kernel without reuse streams
    d["cross_kv_read_bytes_algorithmic"] = cands * kv_bytes
    d["cross_kv_read_bytes_per_pair_form"] = pairs * kv_bytes
    return d


def bench(args):
    import torch
    import torch.nn.functional as F
    from mico_amd import evaluation as Ev
    from mico_amd import functional as Fn
    from mico_amd import ops, runtime
    from mico_amd.model import MiCo, default_cfg
    from mico_amd.weights import synth_state_dict

    assert torch.cuda.is_available(), "rerank_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = MiCo(default_cfg("evaclip02_base", vision_layers=1))          # (only BERT and the ITM head run; the tower is the smallest there is)
    keep = ("multimodal_encoder.", "itm_head.")
    sd = synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items() if k.startswith(keep)}, seed=0)
    model.load_state_dict(sd, strict=False)
    model.to(dev).eval()
    bert = model.multimodal_encoder.bert
    nq, nc, k, E, S = args.nq, args.nc, args.k, args.E, 77
    g = torch.Generator().manual_seed(1)
    # correlated features so that the two directions' shortlists overlap the way a trained model's do: text i is a noisy copy of candidate i % nc
    base = F.normalize(torch.randn(nc, 512, generator=g), dim=-1)
    feat_c = base.to(dev)
    feat_t = F.normalize(base[torch.arange(nq) % nc] + 0.35 * torch.randn(nq, 512, generator=g), dim=-1).to(dev)
    cond16 = torch.empty(nc, E, D, dtype=torch.float16, device=dev)
    for c0 in range(0, nc, 100):
        cond16[c0:c0 + 100] = torch.randn(min(100, nc - c0), E, D, generator=g).to(dev)
    lens = torch.randint(8, 41, (nq,), generator=g)
    ids = torch.zeros(nq, S, dtype=torch.long)
    am = torch.zeros(nq, S, dtype=torch.long)
    for i, n in enumerate(lens.tolist()):
        ids[i, :n] = torch.randint(1000, 30000, (n,), generator=g)
        ids[i, 0], ids[i, n - 1] = 101, 102
        am[i, :n] = 1
    ids, am = ids.to(dev), am.to(dev)
    res = dict(tool="rerank_bench", dtype=args.dtype, pair_batch=args.pair_batch, pair_batch_a=args.pair_batch_a, rounds=args.rounds)
    # plain 16-bit MFMA operands (what bench.py times for BERT): the fp16 parity split would triple the GEMM work, most of all form a's projections
    state = (torch.float16 if args.dtype == "fp16" else torch.bfloat16, False, "full", False, 0, "weights")
    with runtime.using(state), torch.no_grad():
        sim = Fn.matmul_nt(feat_t, feat_c)

        def time_topk(x, reps):
            ops.topk_rows(x, k)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.topk_rows(x, k)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            return dict(rows=x.shape[0], cols=x.shape[1], k=k, us=round(us, 1), gbps=round(x.numel() * 4 / (us * 1e-6) / 1e9, 1))

        res["topk_rows"] = [time_topk(sim, 20)]
        if args.nq >= 1000:                               # the COCO-5k matrix (25 000 texts x 5 000 images, 500 MB): where the one-pass bound is a rate
            res["topk_rows"].append(time_topk(torch.randn(25000, 5000, device=dev), 5))
        top_t2c = ops.topk_rows(sim, k)[1]
        top_c2t = ops.topk_rows(sim.t().contiguous(), k)[1]
        plan = Ev.plan_pairs(top_t2c.cpu(), top_c2t.cpu(), n_text=nq, n_cand=nc)
        P = plan.text.numel()
        text_dev, cand_dev = plan.text.to(dev), plan.cand.to(dev)

        def form_a():
            out = torch.empty(P, dtype=torch.float32, device=dev)
            for p0 in range(0, P, args.pair_batch_a):
                p1 = min(p0 + args.pair_batch_a, P)
                cond = cond16[cand_dev[p0:p1]].float()                        # the per-pair copy of the condition tokens (fp32, as forward takes them)
                seq = bert(input_ids=ids[text_dev[p0:p1]], attention_mask=am[text_dev[p0:p1]], encoder_hidden_states=cond).last_hidden_state
                out[p0:p1] = F.softmax(model.itm_head(seq[:, 0]), dim=1)[:, 1]
            return out

        forms = {"a": form_a,
                 "b": lambda: Ev.score_pairs(model, ids, am, cond16, plan, args.kv_budget_gib * 2 ** 30 if args.kv_budget_gib else None, args.pair_batch, False),
                 "c": lambda: Ev.score_pairs(model, ids, am, cond16, plan, args.kv_budget_gib * 2 ** 30 if args.kv_budget_gib else None, args.pair_batch, True)}
        names = [f for f in args.forms.split(",") if f]
        scores, times, peak, stats = {}, {f: [] for f in names}, {}, {}
        for f in names:                                   # warm every form (weight copies, allocator)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            scores[f] = forms[f]().cpu()
            torch.cuda.synchronize()
            peak[f] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
            if f != "a":
                stats[f] = dict(Ev.score_pairs.last_stats)
            print(f"warm {f}: peak {peak[f]} GiB", flush=True)
        for r in range(args.rounds):
            for f in (names if r % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                forms[f]()
                torch.cuda.synchronize()
                times[f].append(time.perf_counter() - t0)
                print(f"round {r} {f}: {times[f][-1]:.3f} s", flush=True)
        # text rows form c actually runs (sum of pairs x trimmed length over its sub-batches): replay the walk on the host
        am_host, text_host = am.cpu(), plan.text
        trim_rows = 0
        max_cands = (stats.get("c") or stats.get("b") or {}).get("max_cands", nc)
        for cands, p0, p1, _ in Ev.plan_chunks(plan.cand, max_cands):
            for q0 in range(p0, p1, args.pair_batch):
                q1 = min(q0 + args.pair_batch, p1)
                trim_rows += (q1 - q0) * Ev.trimmed_length(am_host[text_host[q0:q1]])
        res["counts"] = shape_counts(P, len(set(plan.cand.tolist())), E, S, trim_rows, nq, nc, k)
        res["counts"]["bert_passes"] = {"a": -(-P // args.pair_batch_a), **{f: s["bert_passes"] for f, s in stats.items()}}
        res["counts"]["chunks"] = {f: s["chunks"] for f, s in stats.items()}
        res["seconds"] = {f: round(statistics.median(t), 3) for f, t in times.items() if t}
        res["runs_s"] = {f: [round(x, 3) for x in t] for f, t in times.items()}
        res["peak_alloc_gib"] = peak
        if "a" in res["seconds"]:
            for f in ("b", "c"):
                if f in res["seconds"]:
                    res[f"a_over_{f}"] = round(res["seconds"]["a"] / res["seconds"][f], 2)
        if "a" in scores:
            for f in ("b", "c"):
                if f in scores:
                    res[f"max_abs_diff_{f}_vs_a"] = float((scores[f] - scores["a"]).abs().max())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def gpu_steps(args):
    """The GPU steps as child processes, each under its own time limit; the first one that fails (or runs out of time) ends the run."""
    import glob
    me = os.path.abspath(__file__)
    small = ["--rounds", "0", "--nq", "250", "--nc", "250", "--out", ""]
    trace = lambda form: ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(args.trace_dir, form), "--",
                          sys.executable, me, "--forms", form] + small
    probe = os.path.join(ROOT, "tools", "probes", "kv_index_locality.py")
    kvloc = os.path.join(args.trace_dir, "kvloc")
    # (counters in a run of their own, never next to a trace)
    pmc = ["rocprofv3", "--pmc", "FETCH_SIZE", "--kernel-include-regex", "attn_fwd", "--output-format", "csv", "-d", kvloc, "--",
           sys.executable, probe, "--launch"]
    steps = [(1500, [sys.executable, me, "--rounds", str(args.rounds), "--out", args.out]), (600, trace("a")), (600, trace("c")), (300, pmc)]
    for limit, cmd in steps:
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT).returncode
        if rc != 0:
            raise SystemExit(f"step failed with exit status {rc}: {' '.join(cmd)} - nothing further is started")
    text = ("# rocprofv3 --kernel-trace --stats over `python tools/rerank_bench.py --rounds 0 --nq 250 --nc 250 --forms <form>`: ONE pass of the form\n"
            "# (a quarter of the bench's rows and columns, same E = 1285, k = 50, sub-batch sizes); a = per-pair, c = indexed with trimmed text rows\n")
    for form in ("a", "c"):
        csvs = sorted(glob.glob(os.path.join(args.trace_dir, form, "**", "*kernel_stats.csv"), recursive=True))
        if not csvs:
            raise SystemExit(f"no kernel_stats.csv under {os.path.join(args.trace_dir, form)}")
        tab = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prof_summary.py"), csvs[-1], "16"], cwd=ROOT, capture_output=True, text=True)
        text += f"\n## form {form}\n" + tab.stdout
    with open(os.path.join(ROOT, "profiles", "rerank_kernels.txt"), "w") as fh:
        fh.write(text)
    print(text)
    loc = subprocess.run([sys.executable, probe, "--report", kvloc], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    with open(os.path.join(ROOT, "profiles", "rerank_kv_locality.json"), "w") as fh:
        fh.write(loc)
    print(loc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--nc", type=int, default=1000)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--E", type=int, default=1285)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--forms", default="a,b,c")
    ap.add_argument("--pair-batch", type=int, default=512, help="pairs per BERT pass of the indexed forms")
    ap.add_argument("--pair-batch-a", type=int, default=256, help="pairs per BERT pass of the per-pair form (its K/V is 47 MB per pair)")
    ap.add_argument("--kv-budget-gib", type=float, default=0, help="K/V budget of a candidate chunk (0: evaluation.default_kv_budget)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_bench.json"))
    ap.add_argument("--gpu-steps", action="store_true")
    ap.add_argument("--trace-dir", default=None, help="where the rocprofv3 steps put their output (default: a fresh temporary directory)")
    args = ap.parse_args()
    if args.gpu_steps:
        if args.trace_dir is None:
            import tempfile
            args.trace_dir = tempfile.mkdtemp(prefix="rerank_trace_")
        gpu_steps(args)
    else:
        bench(args)


if __name__ == "__main__":
    main()
