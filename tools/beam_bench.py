"""Beam search on the host against beam search on the device (BertForMaskedLM.generate(device_search=True)), BERT only: synthetic weights,
synthetic condition tokens, fp16, cached decode, eos_token_id=None (every step is taken).  Three shapes:
    cap    caption evaluation: 64 prompt rows x 3 beams, E = 2056 condition tokens, 40 new tokens, length penalty 0.6;
    demo   inference_demo.py: 1 x 3 beams, E = 257, 40 new tokens;
    qa     question answering: 16 samples with 72 questions in all x 3 beams (ragged condition sets), E = 1285, 30-token questions, 10 new
           tokens, length penalty 1.
Forms: host (the default search), device (done_check_every=1), device4 (done_check_every=4).  Every form is warmed, the rounds rotate the order
of the forms, every timed window ends in a device synchronise; medians and the spread (max - min) over the rounds are reported, together with
the synchronising torch calls per step of the host and the device form (torch.cuda.set_sync_debug_mode("warn"), counted after the prefill)
and whether the token ids agree.  Also mico_beam_topk alone at 192 and 216 rows of 30522 logits next to mico_vocab_sample on the same rows
(which reads a row three times): microseconds per launch and GB/s over the logits' bytes.

    python tools/beam_bench.py [--rounds 5] [--shapes cap demo qa] [--out profiles/beam_bench.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

D, V = 768, 30522


def shape_inputs(name, m, dev):
    """generate()'s arguments of one shape"""
    g = torch.Generator().manual_seed(1)
    if name == "qa":
        samples, E, Lq, new = 16, 1285, 30, 10
        counts = torch.randint(1, 9, (samples,), generator=g).tolist()
        nq = sum(counts)
        cond = torch.randn(samples, E, D, generator=g).to(dev)
        q = torch.randint(1000, 30000, (nq, Lq), generator=g)
        lens = torch.randint(Lq // 3, Lq + 1, (nq,), generator=g)
        kp = (torch.arange(Lq)[None] < lens[:, None]).long()
        prompt = torch.cat([q * kp, torch.full((nq, 1), 101)], dim=1).to(dev)
        mask = m.update_attention_mask(kp[:, None, :].expand(nq, Lq, Lq).contiguous()).to(dev)
        return dict(input_ids=prompt, attention_mask=mask, encoder_hidden_states=cond, rows_per_condition=counts, max_new_tokens=new,
                    length_penalty=1.0), dict(prompt_rows=nq, E=E, new_tokens=new, questions_per_sample=counts)
    rows, E, new = (64, 2056, 40) if name == "cap" else (1, 257, 40)
    cond = torch.randn(rows, E, D, generator=g).to(dev)
    prompt = torch.full((rows, 1), 101, dtype=torch.long, device=dev)
    return dict(input_ids=prompt, attention_mask=prompt.new_ones(rows, 1, 1), encoder_hidden_states=cond, max_new_tokens=new,
                length_penalty=0.6), dict(prompt_rows=rows, E=E, new_tokens=new)


def count_syncs(run):
    """synchronising torch calls during run(), counted from the return of the decode's first model step (the prefill) on"""
    from mico_amd.model.bert import BertForMaskedLM
    state = dict(on=False, n=0)
    real = BertForMaskedLM._model_step

    class AfterPrefill:
        def __init__(self, dec):
            self.dec = dec

        def next_token_logits(self, ids, parent=None):
            out = self.dec.next_token_logits(ids, parent)
            state["on"] = True
            return out

    def hook(message, category, filename, lineno, file=None, line=None):
        state["n"] += state["on"] and "synchroniz" in str(message)

    BertForMaskedLM._model_step = lambda self, *a, **k: AfterPrefill(real(self, *a, **k))
    old = warnings.showwarning
    with warnings.catch_warnings():
        warnings.simplefilter("always")
        warnings.showwarning = hook
        torch.cuda.set_sync_debug_mode("warn")
        try:
            run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
            warnings.showwarning = old
            BertForMaskedLM._model_step = real
    return int(state["n"])


def device_us(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["cap", "demo", "qa"])
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--kernel_reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    args = ap.parse_args()
    from mico_amd import ops, runtime
    from mico_amd.model.bert import BertForMaskedLM, build_tokenizer
    from mico_amd.weights import synth_state_dict

    assert torch.cuda.is_available(), "beam_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BertForMaskedLM()
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0), strict=False)
    m.tokenizer = build_tokenizer()
    m.to(dev).eval()
    forms = dict(host={}, device=dict(device_search=True), device4=dict(device_search=True, done_check_every=4))
    res = dict(tool="beam_bench", dtype="fp16", beams=args.beams, rounds=args.rounds, shapes={})
    with runtime.precision(torch.float16), torch.no_grad():
        for name in args.shapes:
            kw, info = shape_inputs(name, m, dev)
            kw.update(num_beams=args.beams, eos_token_id=None, pad_token_id=0, use_cache=True)
            run = lambda f: m.generate(**kw, **forms[f])
            ids = {f: run(f).cpu() for f in forms}                  # warm every form
            times = {f: [] for f in forms}
            order = list(forms)
            for r in range(args.rounds):
                for f in order[r % 3:] + order[:r % 3]:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(f)
                    torch.cuda.synchronize()
                    times[f].append((time.perf_counter() - t0) * 1e3)
            out = dict(info, decode_rows=info["prompt_rows"] * args.beams)
            for f in forms:
                out[f] = dict(ms_per_decode=round(statistics.median(times[f]), 2), spread_ms=round(max(times[f]) - min(times[f]), 2),
                              runs_ms=[round(t, 2) for t in times[f]])
            steps = info["new_tokens"] - 1                            # (counted after the prefill step)
            for f in ("host", "device", "device4"):
                n = count_syncs(lambda: run(f))
                out[f]["syncs_after_prefill"] = n
                out[f]["syncs_per_step"] = round(n / steps, 2)
            out["ids_equal"] = bool(all(torch.equal(ids["host"], ids[f]) for f in forms))
            out["rows_with_equal_ids"] = int((ids["host"] == ids["device"]).all(dim=1).sum()) if ids["host"].shape == ids["device"].shape else None
            out["device_over_host"] = round(out["device"]["ms_per_decode"] / out["host"]["ms_per_decode"], 4)
            res["shapes"][name] = out
        kern = {}
        for rows in (192, 216):
            g = torch.Generator().manual_seed(rows)
            logits = (3 * torch.randn(rows, V, generator=g)).to(dev)
            bs = (-30 * torch.rand(rows, generator=g)).to(dev)
            u = torch.rand(rows, generator=g).to(dev)
            ids12 = torch.randint(0, V, (rows, 12), generator=g).to(dev)
            nbytes = rows * V * 4
            entry = {}
            for label, fn in (("beam_topk", lambda: ops.beam_topk(logits, bs, args.beams)),
                              ("beam_topk_processors", lambda: ops.beam_topk(logits, bs, args.beams, ids=ids12, repetition_penalty=1.3,
                                                                             no_repeat_ngram_size=2, ban_eos=True, eos_token_id=102)),
                              ("vocab_sample", lambda: ops.vocab_sample(logits, u)),
                              ("torch_log_softmax_topk", lambda: torch.topk((torch.log_softmax(logits, dim=-1) + bs[:, None])
                                                                            .view(rows // args.beams, -1), 2 * args.beams, dim=1))):
                us = device_us(fn, args.kernel_reps)
                entry[label] = dict(us=round(us, 1), gb_per_s=round(nbytes / us / 1e3, 1))
            kern[str(rows)] = entry
        res["kernels"] = dict(cols=V, logits_bytes_per_row=V * 4, rows=kern,
                              note="us per call (allocation of the outputs included), GB/s over one read of the logits")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
