"""One SCST caption fine-tuning step of the text head (BERT + LM head; synthetic weights and condition tokens, fp16), forward and backward,
in two schedules:
    stepwise    the reference's (model/bert.py:1230-1502, sample_scst): one pass WITH grad per generated token over the growing prefix plus
                the appended [MASK] - every pass projects the cross-attention K/V of the condition tokens again and keeps its graph - the
                next token drawn from that pass's logits (mico_vocab_sample), its log-prob from functional.LMHeadLogProbFn on the [MASK]
                row; then one backward through all T graphs.  The parent of this tool's commit has no per-row log-probs, so this form, on
                the same product functions, is the baseline;
    two_stream  BertForMaskedLM.generate_scst: the no-grad cached roll-out (functional.BertDecodeCache), then ONE differentiable pass of
                (P + T - 1) + T rows per caption (sequence_logprobs), then its backward.
Both differentiate sum(advantage[row] * logprobs[row, t]) with the same advantages and uniform numbers, down to the condition tokens.
Default shape: 64 condition sets, E = 1285 condition tokens (g/14: 5 frames x 257), 1 sampled caption each, prompt [CLS], 20 new tokens,
eos_token_id=None (every step is taken).  Every form is warmed, the rounds alternate the order, every timed window ends in a device synchronise.

    python tools/scst_bench.py [--sets 64] [--E 1285] [--new_tokens 20] [--rounds 3] [--out profiles/scst_bench.json]

Prints one JSON line (ms per step, peak allocated memory, rows differentiated and K/V projections per form, the ratio) and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

D = 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--E", type=int, default=1285)
    ap.add_argument("--new_tokens", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scst_bench.json"))
    args = ap.parse_args()
    from mico_amd import functional as Fn, ops, runtime
    from mico_amd.model.bert import BertForMaskedLM, build_tokenizer
    from mico_amd.weights import synth_state_dict

    assert torch.cuda.is_available(), "scst_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BertForMaskedLM()
    sd = synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict(sd, strict=False)
    m.tokenizer = build_tokenizer()
    m.to(dev).eval()          # (no dropout in either form: the two do the same arithmetic)

    R, T = args.sets, args.new_tokens
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(R, args.E, D, generator=g).to(dev).requires_grad_(True)
    noise = torch.rand(R, T, generator=g).to(dev)
    adv = torch.randn(R, generator=g).to(dev)
    prompt = torch.full((R, 1), m.tokenizer.bos_token_id, dtype=torch.long, device=dev)
    pmask = prompt.new_ones(R, 1, 1)

    def stepwise():
        ids, mask, logps = prompt, pmask, []
        for t in range(T):
            inp = m.prepare_inputs_for_generation(ids, mask, cond)
            seq = m.bert(inp["input_ids"], inp["attention_mask"], inp["encoder_hidden_states"]).last_hidden_state
            last = seq[:, -1:, :]
            with torch.no_grad():
                logits = Fn.LMLogitsFn.apply(last.detach().contiguous(), *[p.detach() for p in m._head_params()])[:, 0, :]
                tok, _ = ops.vocab_sample(logits, noise[:, t].contiguous())
            logps.append(Fn.LMHeadLogProbFn.apply(last, tok.view(R, 1), *m._head_params())[:, 0])
            ids, mask = torch.cat([ids, tok.view(R, 1)], dim=1), inp["attention_mask"]
        return ids, torch.stack(logps, dim=1)

    def two_stream():
        return m.generate_scst(prompt, pmask, cond, max_new_tokens=T, eos_token_id=None, pad_token_id=0, sample_noise=noise, use_cache=True)

    forms = {"stepwise": stepwise, "two_stream": two_stream}

    def step(f):
        m.zero_grad(set_to_none=True)
        cond.grad = None
        ids, logp = forms[f]()
        (adv[:, None] * logp).sum().backward()
        return ids, logp.detach()

    res = dict(tool="scst_bench", dtype="fp16", sets=R, E=args.E, new_tokens=T, rounds=args.rounds)
    names = list(forms)
    with runtime.precision(torch.float16):
        outs, times, peak = {}, {f: [] for f in names}, {}
        for f in names:                                # warm every shape
            outs[f] = step(f)
        for f in names:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            step(f)
            torch.cuda.synchronize()
            peak[f] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
        for r in range(args.rounds):
            for f in (names if r % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(f)
                torch.cuda.synchronize()
                times[f].append((time.perf_counter() - t0) * 1e3)
    rows = {"stepwise": sum(1 + t + 1 for t in range(T)), "two_stream": T + T}      # rows with a gradient, per caption (P = 1)
    for f in names:
        res[f] = dict(ms_per_step=round(statistics.median(times[f]), 2), runs_ms=[round(t, 2) for t in times[f]],
                      peak_alloc_gib=round(peak[f], 3), grad_rows_per_caption=rows[f], kv_projections_with_grad=T if f == "stepwise" else 1)
    same = (outs["stepwise"][0] == outs["two_stream"][0]).all(dim=1)
    res["rows_with_equal_ids"] = int(same.sum())
    res["max_logp_diff_on_equal_rows"] = float((outs["stepwise"][1] - outs["two_stream"][1])[same].abs().max()) if bool(same.any()) else None
    res["stepwise_over_two_stream"] = round(res["stepwise"]["ms_per_step"] / res["two_stream"]["ms_per_step"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
