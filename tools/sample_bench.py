"""Sampling decode on the host (BertForMaskedLM.generate(do_sample=True, top_k=10), the captioner_mode call) against the sampling decode on the
device (BertForMaskedLM.sample), BERT only: synthetic weights, synthetic condition tokens, fp16, cached decode, eos [SEP].  The shape is
tools/beam_bench.py's caption evaluation with generate_nums sampled captions per condition set: 64 sets x 3 rows, E = 2056 condition tokens,
40 new tokens.  Forms, all with the same injected uniform numbers:
    host      generate(do_sample=True, top_k=10)
    device    sample(top_k=10)                      (done_check_every=1)
    device4   sample(top_k=10, done_check_every=4)
    nucleus   sample(top_k=0, top_p=0.9, temperature=0.7)
Every form is warmed, the rounds rotate the order of the forms, every timed window ends in a device synchronise; medians and the spread
(max - min) over the rounds are reported, with the synchronising torch calls per step (counted after the prefill) and whether the ids of
host and device agree (asserted).  Also mico_warp_sample alone (top-k mode, nucleus mode, nucleus mode with the processors) next to
mico_vocab_sample and torch's topk + softmax on the same 192 rows of 30522 logits: microseconds per call.

    python tools/sample_bench.py [--rounds 5] [--out profiles/sample_bench.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from beam_bench import D, V, count_syncs, device_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--generate_nums", type=int, default=3)
    ap.add_argument("--cond_tokens", type=int, default=2056)
    ap.add_argument("--new_tokens", type=int, default=40)
    ap.add_argument("--kernel_reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    args = ap.parse_args()
    from mico_amd import ops, runtime
    from mico_amd.model.bert import BertForMaskedLM, build_tokenizer
    from mico_amd.weights import synth_state_dict

    assert torch.cuda.is_available(), "sample_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BertForMaskedLM()
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0), strict=False)
    m.tokenizer = build_tokenizer()
    m.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    sets, gn, T = args.sets, args.generate_nums, args.new_tokens
    rows = sets * gn
    cond = torch.randn(sets, args.cond_tokens, D, generator=g).to(dev)
    prompt = torch.full((sets, 1), 101, dtype=torch.long, device=dev)
    noise = torch.rand(rows, T, generator=g).to(dev)
    kw = dict(input_ids=prompt, attention_mask=prompt.new_ones(sets, 1, 1), encoder_hidden_states=cond, max_new_tokens=T, eos_token_id=102,
              pad_token_id=0, use_cache=True, num_return_sequences=gn, sample_noise=noise)
    forms = dict(host=lambda: m.generate(do_sample=True, top_k=10, **kw), device=lambda: m.sample(top_k=10, **kw),
                 device4=lambda: m.sample(top_k=10, done_check_every=4, **kw),
                 nucleus=lambda: m.sample(top_k=0, top_p=0.9, temperature=0.7, **kw))
    res = dict(tool="sample_bench", dtype="fp16", rounds=args.rounds, sets=sets, generate_nums=gn, decode_rows=rows, E=args.cond_tokens,
               new_tokens=T)
    with runtime.precision(torch.float16), torch.no_grad():
        ids = {f: run().cpu() for f, run in forms.items()}                  # warm every form
        assert torch.equal(ids["host"], ids["device"]) and torch.equal(ids["host"], ids["device4"]), "host and device ids differ"
        times = {f: [] for f in forms}
        order = list(forms)
        for r in range(args.rounds):
            k = r % len(order)
            for f in order[k:] + order[:k]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                forms[f]()
                torch.cuda.synchronize()
                times[f].append((time.perf_counter() - t0) * 1e3)
        steps = max(ids["host"].shape[1] - 2, 1)                             # (counted after the prefill step)
        for f, run in forms.items():
            n = count_syncs(run)
            res[f] = dict(ms_per_decode=round(statistics.median(times[f]), 2), spread_ms=round(max(times[f]) - min(times[f]), 2),
                          runs_ms=[round(t, 2) for t in times[f]], steps=int(ids[f].shape[1] - 1), syncs_after_prefill=n,
                          syncs_per_step=round(n / steps, 2))
        res["ids_equal"] = True
        res["device_over_host"] = round(res["device"]["ms_per_decode"] / res["host"]["ms_per_decode"], 4)
        g = torch.Generator().manual_seed(rows)
        logits = (3 * torch.randn(rows, V, generator=g)).to(dev)
        u = torch.rand(rows, generator=g).to(dev)
        ids12 = torch.randint(0, V, (rows, 12), generator=g).to(dev)
        proc = dict(ids=ids12, repetition_penalty=1.3, no_repeat_ngram_size=2, ban_eos=True, eos_token_id=102)
        kern = {}
        for label, fn in (("warp_sample_top_k_10", lambda: ops.warp_sample(logits, u, top_k=10)),
                          ("warp_sample_top_k_64", lambda: ops.warp_sample(logits, u, top_k=64)),
                          ("warp_sample_top_k_10_top_p", lambda: ops.warp_sample(logits, u, top_k=10, top_p=0.9, temperature=0.7)),
                          ("warp_sample_nucleus", lambda: ops.warp_sample(logits, u, top_p=0.9, temperature=0.7)),
                          ("warp_sample_nucleus_processors", lambda: ops.warp_sample(logits, u, top_p=0.9, temperature=0.7, **proc)),
                          ("warp_sample_top_p_1", lambda: ops.warp_sample(logits, u)),
                          ("vocab_sample", lambda: ops.vocab_sample(logits, u)),
                          ("torch_topk_10_softmax", lambda: torch.softmax(torch.topk(logits, 10, dim=-1)[0], dim=-1))):
            kern[label] = round(device_us(fn, args.kernel_reps), 1)
        res["kernels"] = dict(rows=rows, cols=V, us=kern, note="us per call (allocation of the outputs included)")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
