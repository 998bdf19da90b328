"""L2-miss traffic of the indexed cross-attention forward (mico_attn_params.kv_index) against its algorithmic K/V bytes.

The launch of one re-ranking sub-batch at the bench shape: B pairs sorted by candidate (`--per-cand` consecutive entries read the same K/V
set), H = 12, hd 64, Sk = 1285 keys, Sq = 77 or a trimmed 48 query rows, K/V one layer of the interleaved memory (row stride 12 x 2 x 768).
A workgroup is one (b, h) item with linear id h + 12 b, so the readers of one (set, head) block alternate between two XCDs ((h + 4 b) % 8).

    python tools/probes/kv_index_locality.py --launch                    # what rocprofv3 wraps: 1 warm launch + `--reps` launches per case
    rocprofv3 --pmc FETCH_SIZE --kernel-include-regex attn_fwd --output-format csv -d DIR -- python tools/probes/kv_index_locality.py --launch
    python tools/probes/kv_index_locality.py --report DIR                # FETCH_SIZE (KiB, doubled: gfx950 tallies 128-byte requests at 64 B)
                                                                         # per launch / algorithmic bytes (distinct (set, head) blocks once)
The cases run in a fixed order (CASES), `--reps` launches each after one warm launch; the report groups the counter rows in that order."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, HD, D, L, SK = 12, 64, 768, 12, 1285
CASES = [dict(B=512, Sq=77, per_cand=50), dict(B=512, Sq=48, per_cand=50), dict(B=512, Sq=77, per_cand=1)]
REPS = 3


def launch():
    import torch
    from mico_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for c in CASES:
        B, Sq, pc = c["B"], c["Sq"], c["per_cand"]
        sets = -(-B // pc)
        kv = torch.empty(sets * SK, L * 2 * D, dtype=torch.float16, device=dev).normal_()[:, :2 * D]     # layer 0 of the interleaved memory
        q = torch.randn(B * Sq, D, generator=g).to(torch.float16).to(dev)
        o = torch.empty_like(q)
        lse = torch.empty(B, H, Sq, dtype=torch.float32, device=dev)
        idx = (torch.arange(B) // pc).to(torch.int32).to(dev)
        krs = kv.stride(0)
        for _ in range(1 + REPS):
            ops.attn_fwd(q, kv, kv[:, D:], o, lse, B=B, H=H, Sq=Sq, Sk=SK, hd=HD, scale=HD ** -0.5, q_strides=(Sq * D, D),
                         k_strides=(SK * krs, krs), v_strides=(SK * krs, krs), o_strides=(Sq * D, D), kv_index=idx)
        torch.cuda.synchronize()


def report(d):
    acc = {}
    files = sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True), key=os.path.getmtime)
    for f in files[-1:]:                                                     # (the newest run, should DIR hold several)
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == "FETCH_SIZE" and "attn_fwd" in r["Kernel_Name"]:
                key = int(r.get("Dispatch_Id", len(acc)))
                acc[key] = acc.get(key, 0.0) + float(r["Counter_Value"])      # (summed should a dispatch be reported in several rows)
    rows = sorted(acc.items())
    out = []
    for i, c in enumerate(CASES):
        mine = rows[i * (1 + REPS) + 1:(i + 1) * (1 + REPS)]            # (the warm launch is left out)
        if not mine:
            continue
        fetched = 2.0 * 1024.0 * sum(v for _, v in mine) / len(mine)
        sets = -(-c["B"] // c["per_cand"])
        algorithmic = sets * H * SK * HD * 2 * 2                        # every distinct (set, head) K and V block once, 16-bit
        q_bytes = c["B"] * c["Sq"] * D * 2
        out.append(dict(c, launches=len(mine), fetch_bytes_per_launch=fetched, kv_bytes_algorithmic=algorithmic, q_bytes=q_bytes,
                        kv_bytes_per_entry_form=c["B"] * H * SK * HD * 2 * 2,
                        fetched_over_algorithmic=round((fetched - q_bytes) / algorithmic, 2)))
    print(json.dumps(dict(tool="kv_index_locality", note="FETCH_SIZE doubled (gfx950); the query rows' bytes are taken off before the ratio",
                          cases=out), indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--report", default=None)
    a = ap.parse_args()
    if a.report:
        report(a.report)
    else:
        launch()
