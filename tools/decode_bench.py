"""Caption decode time of BertForMaskedLM.generate with the K/V cache off (the recomputing path) and on (functional.BertDecodeCache),
BERT only: synthetic weights, synthetic condition tokens, fp16, 40 new tokens with eos_token_id=None (both paths take every step).
Configurations:
    captioner  64 sets x 3 sampled rows (captioner_mode: num_return_sequences 3, top-k 10, injected noise), E = 2056 (8 frames x 257)
    cap_eval   64 sets x 3 beams, E = 2056
    demo       1 set x 3 beams, E = 257
The rounds alternate the order of the two paths, every shape is warmed, every timed window is bracketed by device synchronisations.

    python tools/decode_bench.py [--configs captioner,cap_eval,demo] [--rounds 2] [--out profiles/decode_bench.json]

Prints one JSON line (ms per decode and per step, peak allocated memory, equal token ids) and writes it to --out.  For a kernel profile:
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/decode_bench.py --configs captioner --rounds 1 --paths on --out <file>`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CONFIGS = {"captioner": dict(sets=64, rows=3, E=2056, sample=True), "cap_eval": dict(sets=64, rows=3, E=2056, sample=False),
           "demo": dict(sets=1, rows=3, E=257, sample=False)}
NEW = 40


def decode_bytes(sets, rows, E, steps=NEW, L=12, D=768):
    """HBM bytes the cached decode's attention must read: every step streams each set's cross-attention K/V once per layer (16-bit)."""
    return steps * L * sets * E * 2 * D * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="captioner,cap_eval,demo")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--paths", default="off,on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.json"))
    args = ap.parse_args()
    from mico_amd import runtime
    from mico_amd.model.bert import BertForMaskedLM, build_tokenizer
    from mico_amd.weights import synth_state_dict

    assert torch.cuda.is_available(), "decode_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BertForMaskedLM()
    sd = synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict(sd, strict=False)
    m.tokenizer = build_tokenizer()
    m.to(dev).eval()
    paths = args.paths.split(",")
    res = dict(tool="decode_bench", new_tokens=NEW, dtype="fp16", configs={})
    with runtime.precision(torch.float16), torch.no_grad():
        for name in args.configs.split(","):
            c = CONFIGS[name]
            g = torch.Generator().manual_seed(1)
            cond = torch.randn(c["sets"], c["E"], 768, generator=g).to(dev)
            noise = torch.rand(c["sets"] * c["rows"], NEW, generator=g)
            init = torch.full((c["sets"], 1), 101, dtype=torch.long, device=dev)

            def run(cached):
                kw = dict(input_ids=init, attention_mask=init.new_ones(c["sets"], 1, 1), max_new_tokens=NEW, eos_token_id=None, pad_token_id=0,
                          use_cache=cached)
                if c["sample"]:
                    # the recomputing path gets the condition expanded sample-major, as captioner_mode hands it over without the cache
                    enc = cond if cached else cond.repeat_interleave(c["rows"], dim=0).contiguous()
                    return m.generate(encoder_hidden_states=enc, do_sample=True, top_k=10, sample_noise=noise,
                                      num_return_sequences=c["rows"] if cached else 1,
                                      **dict(kw, input_ids=init if cached else init.repeat_interleave(c["rows"], 0),
                                             attention_mask=(init if cached else init.repeat_interleave(c["rows"], 0)).new_ones(
                                                 c["sets"] * (1 if cached else c["rows"]), 1, 1)))
                return m.generate(encoder_hidden_states=cond, num_beams=c["rows"], length_penalty=0.6, **kw)

            ids, times, peak = {}, {p: [] for p in paths}, {}
            for p in paths:                               # warm every shape
                ids[p] = run(p == "on").cpu()
            for p in paths:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                run(p == "on")
                torch.cuda.synchronize()
                peak[p] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
            for r in range(args.rounds):
                for p in (paths if r % 2 == 0 else paths[::-1]):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(p == "on")
                    torch.cuda.synchronize()
                    times[p].append((time.perf_counter() - t0) * 1e3)
            d = dict(sets=c["sets"], rows_per_set=c["rows"], E=c["E"], sampled=c["sample"], cross_kv_bytes_per_decode=decode_bytes(c["sets"], c["rows"], c["E"]))
            for p in paths:
                ms = statistics.median(times[p])
                d[p] = dict(ms_per_decode=round(ms, 2), ms_per_step=round(ms / NEW, 3), runs_ms=[round(t, 2) for t in times[p]],
                            peak_alloc_gib=round(peak[p], 3))
            if "on" in ids and "off" in ids:
                d["ids_equal"] = bool(torch.equal(ids["on"], ids["off"]))
                d["speedup"] = round(d["off"]["ms_per_decode"] / d["on"]["ms_per_decode"], 2)
            res["configs"][name] = d
            print(name, json.dumps(d), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
