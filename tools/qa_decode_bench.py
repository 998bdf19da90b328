"""Answer decode time of question-answering evaluation (MiCo.forward_qa(compute_loss=False) with decode_use_cache) when samples carry
different numbers of questions, BERT only: synthetic weights, synthetic condition tokens, fp16, beam search with eos_token_id=None (every
step is taken).  Both forms use the cached decode (functional.BertDecodeCache):
    expanded   the condition tokens copied once per question and every copy projected to cross-attention K/V (one condition set per
               prompt row: what generate(use_cache=True) could do before it took rows_per_condition);
    ragged     generate(rows_per_condition=...): every sample's tokens projected once, its questions' rows share the K/V through
               mico_attn_decode_ragged.
Default shape: 16 samples, 1 - 8 questions each (seeded), E = 1285 condition tokens (g/14: 5 frames x 257), 30-token questions, 3 beams,
10 new tokens.  Every shape is warmed, the rounds alternate the order of the two forms, every timed window ends in a device synchronise.

    python tools/qa_decode_bench.py [--samples 16] [--E 1285] [--rounds 5] [--out profiles/qa_decode_bench.json]

Prints one JSON line (ms per decode, peak allocated memory, K/V projection counts and bytes, whether the token ids agree) and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

L, D = 12, 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--max_questions", type=int, default=8)
    ap.add_argument("--E", type=int, default=1285)
    ap.add_argument("--Lq", type=int, default=30)
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--new_tokens", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qa_decode_bench.json"))
    args = ap.parse_args()
    from mico_amd import runtime
    from mico_amd.model.bert import BertForMaskedLM, build_tokenizer
    from mico_amd.weights import synth_state_dict

    assert torch.cuda.is_available(), "qa_decode_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BertForMaskedLM()
    sd = synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict(sd, strict=False)
    m.tokenizer = build_tokenizer()
    m.to(dev).eval()

    g = torch.Generator().manual_seed(1)
    counts = torch.randint(1, args.max_questions + 1, (args.samples,), generator=g).tolist()
    nq = sum(counts)
    cond = torch.randn(args.samples, args.E, D, generator=g).to(dev)
    q = torch.randint(1000, 30000, (nq, args.Lq), generator=g)
    lens = torch.randint(args.Lq // 3, args.Lq + 1, (nq,), generator=g)
    kp = (torch.arange(args.Lq)[None] < lens[:, None]).long()
    prompt = torch.cat([q * kp, torch.full((nq, 1), 101)], dim=1).to(dev)
    mask = m.update_attention_mask(kp[:, None, :].expand(nq, args.Lq, args.Lq).contiguous()).to(dev)
    own = torch.arange(args.samples).repeat_interleave(torch.tensor(counts)).to(dev)
    kw = dict(input_ids=prompt, attention_mask=mask, max_new_tokens=args.new_tokens, num_beams=args.beams, eos_token_id=None, pad_token_id=0,
              length_penalty=1.0, use_cache=True)

    def run(form):
        if form == "expanded":
            return m.generate(encoder_hidden_states=cond[own].contiguous(), **kw)       # (the copy is part of this form's cost)
        return m.generate(encoder_hidden_states=cond, rows_per_condition=counts, **kw)

    forms = ["expanded", "ragged"]
    kv_bytes = lambda sets: sets * args.E * L * 2 * D * 2
    res = dict(tool="qa_decode_bench", dtype="fp16", samples=args.samples, questions_per_sample=counts, questions=nq, E=args.E, Lq=args.Lq,
               beams=args.beams, new_tokens=args.new_tokens, rounds=args.rounds, decode_rows=nq * args.beams)
    with runtime.precision(torch.float16), torch.no_grad():
        ids, times, peak = {}, {f: [] for f in forms}, {}
        for f in forms:                                # warm every shape
            ids[f] = run(f).cpu()
        for f in forms:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            run(f)
            torch.cuda.synchronize()
            peak[f] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
        for r in range(args.rounds):
            for f in (forms if r % 2 == 0 else forms[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(f)
                torch.cuda.synchronize()
                times[f].append((time.perf_counter() - t0) * 1e3)
    for f, sets in (("expanded", nq), ("ragged", args.samples)):
        res[f] = dict(ms_per_decode=round(statistics.median(times[f]), 2), runs_ms=[round(t, 2) for t in times[f]],
                      peak_alloc_gib=round(peak[f], 3), kv_projections=sets, cross_kv_bytes=kv_bytes(sets))
    res["ids_equal"] = bool(torch.equal(ids["expanded"], ids["ragged"]))
    res["rows_with_equal_ids"] = int((ids["expanded"] == ids["ragged"]).all(dim=1).sum()) if ids["expanded"].shape == ids["ragged"].shape else None
    res["expanded_over_ragged"] = round(res["expanded"]["ms_per_decode"] / res["ragged"]["ms_per_decode"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
