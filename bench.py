#!/usr/bin/env python
"""bench.py - MiCo omni-modal alignment step (ViT-g/14 fwd+bwd) on N MI355X GPUs of one node.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus 1 --steps 5 --warmup 2 --full                  (also every figure beyond the headline, see below)
    python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs DIR      (also the last timed step's outputs as DIR/*.npy)
    python bench.py --gpus 8 --steps 20 --warmup 3          (launches its own 8 ranks, one per GPU, when not already under torchrun)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Workload (default `--workload omni`): ONE RANK'S SHARE of BASELINE.json configs[3], the configuration the metric ("omni-modal
samples/sec/GPU ... at 1/2/4/8 MI355X") is quoted on - per GPU b = 64 samples of image (1 frame) + video (8 frames) + depth (1 frame)
+ audio (4 spectrogram windows of 224x224) + text (77 tokens), i.e. 14 ViT-g/14 tower frames per sample, 896 per GPU; synthetic inputs
resident in HBM, random-init weights of the real architecture (EVA01-CLIP-g/14 tower shared by all four modalities, BERT-base with
cross-attention); one step = forward + backward of the alignment loss "ret%tva%tvd_cap%tva" (ITC + ITM with in-batch hard negatives
for both sub-tasks + causal masked-caption LM; step-B of SURVEY.md section 8d).  The N = 1 line is therefore the same workload as the
N = 8 line (weak scaling: every rank runs this on its own shard, the contrastive features are exchanged with one packed RCCL
all-gather, hard-negative condition rows with an index-then-fetch all-to-all, gradients averaged with bucketed all-reduces overlapped
with the backward).  `secondary.configs2_img_aud_txt` is BASELINE configs[2] (image + audio + text, b = 64: rounds 1-3's headline)
timed in the same run with --full; `--workload img_aud_txt` makes it the headline again.

Precision of the timed run (--dtype): fp16 MFMA operands, fp32 accumulation / residual stream / statistics - the 16-bit type the
reference's own trainer runs in (fp16 autocast, data/utils/pipeline.py:43) at the bf16 MFMA rate.  `parity` in the --full line holds
max|out - ref| / max|ref| of exactly this configuration against the reference-generated goldens (tests/golden/vit_g14_*.pt), measured
in the same process after the timed region - ViT tokens / feat_v, BERT sequence outputs and loss, feat_t / sim logits / ITM scores of the
facade and the three alignment losses; `parity_config` is the same step timed in the configuration with margin under the 1e-3 gate (fp16
with hi/lo-split weights: 2 k-segments per forward GEMM) next to it.

One JSON line on rank 0: the contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step = milliseconds per timed step,
steps, warmup, ...) and
  roofline     - the dominant kernel (MFMA GEMM) timed per launch with HIP events inside the timed region, and the step's MFMA fraction.
A plain run does nothing else: set-up, --warmup untimed steps, exactly --steps timed ones, the line.  --full adds, after the timed steps:
  cpu_baseline - the CPU oracle (oracle/mico_oracle.py, a restatement of the reference parity-locked to it) timed on the
                 host cores on a bounded sample of the same workload plus the BASELINE.md section 4 anchors (rank 0, N = 1 only);
  parity / parity_config / secondary / droppath_ab / comm - see above and main().
--dump-outputs DIR writes what the last timed step computed (losses, a seeded sample of every parameter gradient and their norms; see
dump_outputs) as .npy files; inputs and weights are fixed by seeds, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic forward GF / sample for step-B at config-3 shapes: 2 * MAC of every
# GEMM incl. attention, LM head only where a loss consumes it; fwd+bwd = 3 x fwd
ALG_TFLOP_PER_SAMPLE = {"vitg_img1_aud4_txt77_stepB": 8.74, "vitg_omni14_txt77": 24.04, "vitg_vid8_cap": 13.08, "vitb16_img1_txt77_stepA": 0.1453}
# forward GF of ONE tower block on one frame and the block count: what stochastic depth removes from the executed work
TOWER_BLOCK_GF = {"evaclip01_giant": (40, 13.341), "evaclip02_base": (12, 2.908)}
MFMA_PEAK_TFLOPS = 2500.0   # dense bf16/fp16, /opt/skills/guides/MI355X_MICROARCH.md

PRECISIONS = {   # --dtype -> (torch dtype, split_fp16, split_mode, description)
    "fp8": ("bfloat16", False, "full", "block-scaled MX fp8 (e4m3, E8M0 per 32) MFMA for the forward and input-gradient GEMMs of the towers and "
                                       "BERT's large projections; weight gradients, attention and everything else as bf16"),
    "fp16": ("float16", False, "full", "fp16 MFMA operands, fp32 accumulate / residual stream / LN / softmax; forward GEMMs of the first 4 of the "
                                       "40 tower blocks as x W_hi + x W_lo (runtime.CFG.head_split_blocks)"),
    "fp16-plain": ("float16", False, "full", "fp16 MFMA operands (plain everywhere), fp32 accumulate / residual stream / LN / softmax"),
    "bf16": ("bfloat16", False, "full", "bf16 MFMA operands, fp32 accumulate / residual stream / LN / softmax"),
    "fp16-split-w": ("float16", True, "weights", "fp16 MFMA, forward GEMMs x W_hi + x W_lo (weights hi/lo split, 2 k-segments)"),
    "fp16-split": ("float16", True, "full", "fp16 MFMA, forward GEMMs x_hi W_hi + x_lo W_hi + x_hi W_lo (3 k-segments)"),
}


HEAD_SPLIT_BLOCKS = 4
# Test switches for the N > 1 launch path on a 1-GPU box (tests/test_bench_launch_gpu.py): every rank on device 0, the process group on gloo (it
# carries CUDA tensors; a 1-GPU box cannot host two RCCL ranks).  Never set by the driver: a line produced with them says so (`comm.backend`).
ONE_DEVICE = os.environ.get("MICO_BENCH_ONE_DEVICE") == "1"
BACKEND = os.environ.get("MICO_BENCH_BACKEND", "nccl")


def release_memory():
    """Between the measurements of one process: drop what the previous one left (autograd graphs are reference cycles: the collector first, then the
    caching allocator's blocks), so that the next measurement's tower plan (functional.tower_plan prices the FREE device memory) sees what a
    process of its own would see - the parity_config step of round 5's first collection ran 23 % slower in-process than stand-alone."""
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="samples per GPU")
    ap.add_argument("--vision", default="evaclip01_giant")
    ap.add_argument("--layers", type=int, default=None, help="truncate the ViT (debug only; invalidates the metric)")
    ap.add_argument("--dtype", default="fp16", choices=sorted(PRECISIONS))
    ap.add_argument("--task", default=None)
    ap.add_argument("--workload", default="omni", choices=["img_aud_txt", "omni", "vid_cap_fp8", "b16_img_txt"],
                    help="omni (default) = one rank's share of BASELINE configs[3], the configuration the metric is quoted on: image + video "
                         "(9 vision frames) + depth + audio (4) + text, 14 tower frames/sample, b = 64/GPU; img_aud_txt = BASELINE configs[2] "
                         "(image + audio + text, 5 frames/sample); vid_cap_fp8 = one rank of configs[4]: 8 video frames + BERT generative head "
                         "(CAP), b = 32, --dtype fp8; b16_img_txt = BASELINE configs[1]: ViT-B/16 (EVA02-CLIP-B/16) image + text contrastive "
                         "step (step-A: encoders + heads + ITC), b = 256")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--diet", type=int, default=None, help="force the tower's saved-activation level (0 / 1 / 2 / 3; default: mico_amd.functional.tower_plan decides)")
    ap.add_argument("--diet-mlp-blocks", type=int, default=0, help="with --diet 3: the last n tower blocks keep their MLP intermediates")
    ap.add_argument("--no-comm", action="store_true", help="N = 1: skip the extra steps on a one-rank RCCL group (the `comm` object)")
    ap.add_argument("--no-extras", action="store_true", help="skip parity / parity_config / secondary (only the headline measurement)")
    ap.add_argument("--all-precisions", action="store_true", help="also time fp16-plain and fp8 on the same step (`other_precisions`)")
    ap.add_argument("--cpu-batch", type=int, default=1)
    ap.add_argument("--eval-mode", action="store_true", help="disable DropPath (parity-style run)")
    ap.add_argument("--gemm-detail", action="store_true", help="print a per-shape table of the timed GEMM launches to stderr")
    ap.add_argument("--no-gemm-timer", action="store_true", help="A/B switch: no per-launch HIP events around the GEMMs (roofline is then null)")
    ap.add_argument("--optimizer", action="store_true",
                    help="also run the AdamW step (mico_amd.optim, SURVEY section 8 row f4) inside the timed step: a full training step, "
                         "beyond the metric's fwd+bwd definition")
    ap.add_argument("--no-bert-dropout", action="store_true", help="A/B switch: BERT dropout probabilities set to 0 (invalidates the metric)")
    ap.add_argument("--direct-backward", action="store_true",
                    help="A/B switch: the direct form of the step (every BERT graph built, one backward over all of it) instead of MiCo.forward("
                         "backward_scale=1.0), which differentiates the BERT passes one condition set at a time inside the forward (same values and "
                         "gradients, ~25 GiB lower peak: room for every tower block's MLP pre-activation)")
    ap.add_argument("--dense-droppath", action="store_true",
                    help="evaluate dropped residual branches too and multiply them by 0 (the reference's schedule) instead of skipping them")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: `comm` (N = 1: extra steps on a one-rank RCCL group), the in-run `parity` "
                         "against the goldens, `secondary`, `droppath_ab`, `parity_config` / `other_precisions` and `cpu_baseline` (each still "
                         "switched off by its --no-* flag).  Without it a run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy: the losses (float64) and a fixed, "
                         "seeded sample of every parameter gradient (grad_sample.npy, float32) with each gradient's norm (grad_norm.npy, float64)")
    return ap.parse_args()


def cpu_model_string():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sd_cpu, args):
    """The CPU oracle on the host cores.  `value`: the bench's own step (same task, same per-sample shapes) at --cpu-batch samples,
    BASELINE.md section 4's protocol - one warm-up step + 3 timed steps, median (one omni sample is ~25 s of CPU work per step).
    `anchors`: the BASELINE.md section 4 shapes - config 2 (ViT-B/16 image + text contrastive step) at bs 8, config 3's image + text
    sub-step (ViT-g/14) at bs 2, config 1 (single-image ViT-g/14 encode) - same protocol.  32 threads: PyTorch's CPU GEMMs on this path
    stop scaling (and regress badly) far below the 256 hardware threads of the GPU box's host - a first run with all 256 threads took
    1292 s for a b = 2 sample."""
    from oracle import mico_oracle as O
    from mico_amd.weights import synth_inputs, synth_state_dict
    from mico_amd.model import MiCo, default_cfg
    import random
    ncores = min(32, os.cpu_count() or 1)
    torch.set_num_threads(ncores)
    arch = O.ARCHS[args.vision]
    b = args.cpu_batch

    def tied(sd):
        sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        sd["multimodal_encoder.cls.predictions.decoder.weight"] = sd["multimodal_encoder.bert.embeddings.word_embeddings.weight"]
        return sd

    def timed(fn, n=3, bound_s=60.0):
        t = time.time()
        fn()
        if time.time() - t > bound_s:     # a pathologically slow host: keep the run bounded, say so in `sample` (len(ts) == 1)
            n = 1
        ts = []
        for _ in range(n):
            t = time.time()
            fn()
            ts.append(time.time() - t)
        return statistics.median(ts), ts

    inp = synth_inputs(dict(b=b, **WORKLOADS[args.workload]["shape"]), seed=99)
    sd = tied(sd_cpu)
    mi, lab = O.token_masker(inp["input_ids"], 0.6, random.Random(0))
    idx = torch.arange(b).roll(1)
    injected = {st: dict(neg_cond_idx=idx, neg_text_idx=idx) for st in ("tva", "tvd", "tv")}
    injected["cap"] = dict(masked_ids=mi, labels=lab)

    def own_step():
        for v in sd.values():
            v.grad = None
        out, _ = O.mico_forward(sd, arch, inp, args.task, dict(itm_ratio=0.1), injected=injected)
        sum(out.values()).backward()

    dt, all_dt = timed(own_step)
    res = dict(value=b / dt, unit="samples/s", cores=ncores, kind="port", cpu=cpu_model_string(), host_threads=os.cpu_count(),
               sample=f"oracle/mico_oracle.py fp32, same step ({args.task}) at b={b} ({WORKLOADS[args.workload]['frames']} frames + 77 tokens "
                      f"per sample), 1 warm-up + {len(all_dt)} timed steps, median {dt:.1f} s (timed: {', '.join(f'{t:.1f}' for t in all_dt)} s) on {ncores} threads")

    def itc_step(vt, sdx, bs):
        inpx = synth_inputs(dict(b=bs, vision=1, S=77), seed=98)

        def f():
            for v in sdx.values():
                v.grad = None
            o, _ = O.mico_forward(sdx, O.ARCHS[vt], inpx, "ret%tv", dict(itm_ratio=0.1),
                                  injected={"tv": dict(neg_cond_idx=torch.arange(bs).roll(1), neg_text_idx=torch.arange(bs).roll(1))})
            o["loss_itc"].backward()
        return f

    anchors = {}
    mb = MiCo(default_cfg("evaclip02_base"))
    sdb = tied(synth_state_dict({k: tuple(v.shape) for k, v in mb.state_dict().items()}, seed=0))
    del mb
    t, _ = timed(itc_step("evaclip02_base", sdb, 8))
    anchors["config2_vitb16_img_txt_itc_bs8"] = dict(samples_per_s=8 / t, median_step_s=t)
    del sdb
    t, _ = timed(itc_step(args.vision, sd, 2))
    anchors["config3_vitg14_img_txt_itc_bs2"] = dict(samples_per_s=2 / t, median_step_s=t)
    px = synth_inputs(dict(b=1, vision=1, S=0), seed=97)["vision_pixels"]

    def enc():
        with torch.no_grad():
            O.encode_batch(sd, arch, dict(vision_pixels=px))
    t, _ = timed(enc)
    anchors["config1_vitg14_single_image_encode"] = dict(samples_per_s=1 / t, median_step_s=t)
    res["anchors"] = anchors
    res["anchors_protocol"] = "BASELINE.md section 4: fp32, 1 warm-up + 3 timed steps, median"
    return res


WORKLOADS = {
    "img_aud_txt": dict(shape=dict(vision=1, audio=4, S=77), task="ret%tva_cap%tva", key="vitg_img1_aud4_txt77_stepB", frames=5),
    "omni": dict(shape=dict(vision=9, depth=1, audio=4, S=77), task="ret%tva%tvd_cap%tva", key="vitg_omni14_txt77", frames=14),
    "vid_cap_fp8": dict(shape=dict(vision=8, S=77), task="cap%tv", key="vitg_vid8_cap", frames=8, batch=32, dtype="fp8"),
    # BASELINE configs[1]: step-A of SURVEY.md section 8d (all encoders + heads + packed all-gather + ITC, backward) - the task prefix "itc" is
    # this repo's name for MiCo.forward's contrastive-only objective (ret without the ITM passes)
    "b16_img_txt": dict(shape=dict(vision=1, S=77), task="itc%tv", key="vitb16_img1_txt77_stepA", frames=1, batch=256, vision="evaclip02_base"),
}


def set_precision(name):
    from mico_amd import runtime
    dt, split, mode, _ = PRECISIONS[name]
    runtime.set_compute_dtype(getattr(torch, dt))
    runtime.CFG.split_fp16, runtime.CFG.split_mode = split, mode
    runtime.CFG.fp8 = name == "fp8"
    runtime.CFG.head_split_blocks = HEAD_SPLIT_BLOCKS if name == "fp16" else 0
    runtime.clear_weight_cache()


def measure_parity(model, dev):
    """max|out - ref| / max|ref| of the ACTIVE precision configuration against the reference-generated goldens (tests/golden/*.pt,
    oracle/make_golden.py), the tensors SURVEY section 8d gates at 1e-3: (i) final-LN tokens - the depth-2 g/14 tower on 2 images and the
    full 40-block g/14 (needs the bench's full-depth model); (ii) the L2-normalised 512-d feat_v / feat_t; (iii) the sim logits;
    (iv) scalar losses (relative) - plus BERT's sequence outputs in its three mask modes and the ITM score.  The depth-2 model is built
    here with the same weight generator as the goldens; BERT is depth-independent."""
    import torch.nn.functional as F
    from mico_amd.model import MiCo, default_cfg
    from mico_amd.weights import synth_state_dict, synth_inputs
    from mico_amd.functional import l2_normalize
    from tests.common import golden as load     # (joins the fixtures stored in pieces)
    rel = lambda a, r: ((a.detach().float().cpu() - r.float()).abs().max() / r.float().abs().max().clamp_min(1e-20)).item()
    out = {}
    was_training = model.training
    try:
        fx = load("vit_g14_d2.pt")
        m2 = MiCo(default_cfg("evaclip01_giant", vision_layers=2))
        m2.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m2.state_dict().items()}, 0), strict=False)
        m2.to(dev).eval()
        g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
        x = torch.randn((2, 3, 224, 224), generator=g)
        with torch.no_grad():
            o = m2.vision_encoder.visual(x.to(dev), return_all_features=True).float().cpu()
        out["vit_g14_depth2_tokens"] = ((o - fx["out"]).abs().max() / fx["out"].abs().max()).item()
        # ---- BERT (self-only, 2-D-mask cross-attention, causal cross-attention + LM head + CE): tests/golden/bert.pt
        fx = load("bert.pt")
        g = torch.Generator().manual_seed(fx["meta"]["seed"])
        b, S, E = fx["meta"]["b"], fx["meta"]["S"], fx["meta"]["E"]
        ids = torch.randint(1000, 30000, (b, S), generator=g)
        ids[:, 0] = 101
        mask = (torch.arange(S)[None] < fx["meta"]["lens"][:, None]).long()
        ids = ids * mask
        cond = torch.randn((b, E, 768), generator=g)
        ids, mask, cond = ids.to(dev), mask.to(dev), cond.to(dev)
        me = m2.multimodal_encoder
        with torch.no_grad():
            out["bert_self_seq"] = rel(me(input_ids=ids, attention_mask=mask).sequence_output, fx["self_seq"])
            out["bert_cross_seq"] = rel(me(input_ids=ids, attention_mask=mask, encoder_hidden_states=cond).sequence_output, fx["cross_seq"])
            m3 = torch.tril(mask.unsqueeze(1).expand(-1, S, -1)).contiguous()
            oc = me(input_ids=ids, attention_mask=m3, encoder_hidden_states=cond, labels=fx["labels"].to(dev))
            out["bert_causal_seq"] = rel(oc.sequence_output, fx["causal_seq"])
            out["bert_causal_loss"] = abs(oc.loss.item() - fx["causal_loss"].item()) / fx["causal_loss"].item()
        # ---- facade: feat_v / feat_t / sim logits / ITM score (tests/golden/facade_g14_d2.pt, 4 frames per modality)
        fx = load("facade_g14_d2.pt")["n4"]
        inp = {k: v.to(dev) for k, v in synth_inputs(dict(b=2, vision=4, audio=4, depth=1, S=20), seed=100).items()}
        with torch.no_grad():
            vo = m2.forward_vision_encoder(inp["vision_pixels"])
            fv = l2_normalize(m2.contra_head_v(m2.pool_vision_for_contra(vo)))
            to = m2.forward_multimodal_encoder(inp["input_ids"], inp["attention_mask"]).sequence_output
            ft = l2_normalize(m2.contra_head_t(m2.pool_text_for_contra(to)))
            cv = m2.get_multimodal_forward_input_vision(vo)
            so = m2.forward_multimodal_encoder(inp["input_ids"], inp["attention_mask"], cv).sequence_output
            score = F.softmax(m2.itm_head(so[:, 0]), dim=1)[:, 1]
        out["facade_feat_v"] = rel(fv, fx["feat_v"])
        out["facade_feat_t"] = rel(ft, fx["feat_t"])
        out["facade_sim_t2v_abs"] = (ft @ fv.t() - fx["sim_t2v"].to(dev)).abs().max().item()     # cosine logits in [-1, 1]: absolute
        out["facade_itm_score"] = rel(score, fx["itm_score_full"])
        # ---- the alignment step's three losses with the reference's injected draws (tests/golden/loss_g14_d2.pt, W = 1)
        fx = load("loss_g14_d2.pt")
        r = fx["W1"]
        batch = {k: v.to(dev) for k, v in synth_inputs(dict(b=fx["meta"]["b"], vision=2, audio=1, S=12), seed=1234).items()}
        batch["_injected"] = {st: {k: r["inj"][st][k] for k in ("neg_cond_idx", "neg_text_idx")} for st in ("tva", "tv")}
        batch["_injected"]["cap"] = r["inj"]["cap"]
        lo = m2(batch, fx["meta"]["task"], compute_loss=True)
        for k, v in r["losses"].items():
            out[k + "_rel"] = abs(lo[k].item() - v.item()) / max(abs(v.item()), 1e-6)
        del m2
        if model.config.get("vision_layers") is None and model.config.vision_encoder_type == "evaclip01_giant":
            fx = load("vit_g14_full.pt")
            g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
            x = torch.randn((1, 1, 3, 224, 224), generator=g).to(dev)
            model.eval()
            with torch.no_grad():
                o = model.forward_vision_encoder(x)
                feat = l2_normalize(model.contra_head_v(model.pool_vision_for_contra(o))).float().cpu()
            out["vit_g14_full_token_rows"] = ((o[0, 0, [0, 1, 128, 256]].float().cpu() - fx["rows"]).abs().max() / fx["amax"]).item()
            out["vit_g14_full_feat_v"] = ((feat - fx["feat_v"]).abs().max() / fx["feat_v"].abs().max()).item()
    finally:
        model.train(was_training)
    out["worst"] = max(v for v in out.values() if isinstance(v, float))
    out["metric"] = "max|out - ref| / max|ref| vs reference fp32 CPU outputs (tests/golden, generated by oracle/make_golden.py); losses relative"
    out["gate"] = 1e-3
    return out


def build_model(cfg, seed=0, workers=8):
    """MiCo(cfg) on the host with the synthetic weights loaded: the module and its state dict exactly as a serial
    `MiCo(cfg)` + `synth_state_dict(..., seed)` + `load_state_dict` give them, in a fraction of the time.  The module is built in one
    thread - the only consumer of torch's host generator meanwhile, so it draws what a serial build draws and the steps after it see the
    same stochastic-depth and dropout draws - while the weights, each from its own (seed, name) generator, are synthesised by the
    others; the shapes come from a build on the meta device, which draws nothing."""
    from concurrent.futures import ThreadPoolExecutor
    from mico_amd.model import MiCo
    from mico_amd.weights import synth_state_dict
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in MiCo(cfg).state_dict().items()}
    names = list(shapes)
    chunks = [{n: shapes[n] for n in names[i::workers]} for i in range(workers)]
    with ThreadPoolExecutor(1) as one, ThreadPoolExecutor(workers) as pool:
        fut = one.submit(MiCo, cfg)
        parts = list(pool.map(lambda c: synth_state_dict(c, seed, tie_lm_head=False), chunks))
        model = fut.result()
    merged = {}
    for p in parts:
        merged.update(p)
    sd = {n: merged[n] for n in names if n in merged}
    # the LM head's ties, as synth_state_dict makes them
    w, d = "multimodal_encoder.bert.embeddings.word_embeddings.weight", "multimodal_encoder.cls.predictions.decoder.weight"
    if w in sd and d in sd:
        sd[d] = sd[w]
    b, db = "multimodal_encoder.cls.predictions.bias", "multimodal_encoder.cls.predictions.decoder.bias"
    if b in sd and db in sd:
        sd[db] = sd[b]
    model.load_state_dict(sd, strict=False)
    return model, sd


GRAD_SAMPLE = 4096     # gradient elements per parameter in grad_sample.npy


def dump_outputs(path, model, losses):
    """What the last timed step handed its caller: the losses and every parameter gradient.  The gradients (~1.2 G elements) are
    represented by a fixed sample - GRAD_SAMPLE positions per parameter drawn by a generator seeded with 0, parameters in
    named_parameters() order; a parameter without a gradient contributes zeros - and by each gradient's float64 norm: ~8 MB for ViT-g/14."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for k, v in losses.items():
        np.save(os.path.join(path, f"{k}.npy"), np.asarray(float(v), dtype=np.float64))
    g = torch.Generator().manual_seed(0)
    samples, norms = [], []
    for _, p in model.named_parameters():
        n = p.numel()
        idx = torch.randint(n, (GRAD_SAMPLE,), generator=g) if n > GRAD_SAMPLE else torch.arange(n)
        gr = p.grad
        if gr is None:
            samples.append(torch.zeros(len(idx), dtype=torch.float32))
            norms.append(torch.zeros((), dtype=torch.float64))
            continue
        gr = gr.detach().reshape(-1)
        samples.append(gr[idx.to(gr.device)].float())
        norms.append(torch.linalg.vector_norm(gr, dtype=torch.float64))
    np.save(os.path.join(path, "grad_sample.npy"), torch.cat([s.cpu() for s in samples]).numpy())
    np.save(os.path.join(path, "grad_norm.npy"), torch.stack([t.cpu() for t in norms]).numpy())


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` (N > 1) outside torchrun: become the launcher - one process per GPU over RCCL, same arguments."""
    n = torch.cuda.device_count()
    if n < args.gpus and not ONE_DEVICE:
        sys.exit(f"bench.py: --gpus {args.gpus} but only {n} GPU(s) are visible")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    port = 29500 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


KERNELS = {0: "gemm_kernel<T,{ta},{tb},TileCfg<128,128,2,2,64,2>>", 1: "gemm_kernel<T,{ta},{tb},TileCfg<256,256,2,4,32,4>>",
           2: "gemm_pc_kernel<T,{ta},{tb},32>", 3: "gemm_w4_kernel<T,{ta},{tb}>", 4: "gemm_mx8_kernel<T> (fp8 e4m3 x E8M0/32, v_mfma_scale_f32_16x16x128)",
           5: "gemm_persist_kernel<T,{ta},{tb}> (256x256 8-wave ping-pong, persistent)",
           6: "gemm_kernel<T,{ta},{tb},TileCfg<256,128,2,2,32,3>> (two workgroups per CU)",
           7: "gemm_mid_kernel<T,{tb}> (256x128x64 unit ring, two workgroups per CU)",
           8: "gemm_p8_kernel<T,{tb}> (256x256x64, 8 phases per K-tile, half-tile DMA stream)"}
ROLE = {(0, 0): "y = x W^T (forward)", (0, 1): "dx = dy W", (1, 1): "dW = dy^T x", (1, 0): "x^T W"}
WORKLOAD_TEXT = {
    "img_aud_txt": "BASELINE.json configs[2]: ViT-g/14 image(1)+audio(4x224^2 mel windows)+text(77) fwd+bwd, b={b}/GPU, task {task} (ITC+ITM+CAP)",
    "omni": "BASELINE.json configs[3] per-rank share: ViT-g/14 image(1)+video(8)+depth(1)+audio(4)+text(77) fwd+bwd, 14 tower frames/sample, "
            "b={b}/GPU, task {task} (ITC+ITM for tva and tvd, CAP)",
    "vid_cap_fp8": "BASELINE.json configs[4] per-rank share: ViT-g/14 video (8 x 224^2 frames) + BERT cross-attention generative head (CAP), "
                   "b={b}/GPU, task {task}, fp8 MFMA",
    "b16_img_txt": "BASELINE.json configs[1]: ViT-B/16 (EVA02-CLIP-B/16: RoPE + sub-LN + SwiGLU) image(1)+text(77) contrastive fwd+bwd, b={b}/GPU, "
                   "task {task} (step-A: encoders + heads + ITC)",
}


def kname(key):
    ta, tb, kk = key
    if kk == 4:
        return KERNELS[kk] + " : y = x W^T and dx = dy (W^T)^T"
    return KERNELS[kk].format(ta=str(bool(ta)).lower(), tb=str(bool(tb)).lower()) + " : " + ROLE[(ta, tb)]


def executed_tflop_per_sample(wname, task, kept, share_kv, eval_mode):
    """Algorithmic fwd+bwd TFLOP per sample that the engine executes.  Stochastic depth: a dropped (block, branch, frame) contributes
    exactly zero to values and gradients, so the engine does not evaluate it - the ViT-block share (frames x 40 blocks x 13.341 GF x 3) is
    scaled by the kept fraction of this run's draws.  Shared cross-attention K/V (runtime.CFG.share_cross_kv): the reference projects the
    condition tokens in every BERT pass (ITM triplet = 3 sets, captioning pass = 1), the engine once per distinct set (own + negative):
    12 layers x saved sets x E x 2*768*1536 flop x 3 (fwd + dX + dW)."""
    wl = WORKLOADS[wname]
    nominal = ALG_TFLOP_PER_SAMPLE.get(wl["key"])
    if nominal is None:
        return None, None
    nblk, blk_gf = TOWER_BLOCK_GF[wl.get("vision", "evaclip01_giant")]
    executed = nominal - wl["frames"] * nblk * blk_gf * 3 / 1e3 * (1.0 - kept)
    if share_kv and not eval_mode and task == wl["task"]:
        if wname == "img_aud_txt":        # tva: 4 sets -> 2, E = 5 x 257
            executed -= 12 * 2 * 1285 * 2 * 768 * 1536 * 3 / 1e12
        elif wname == "omni":             # tva (E = 13 x 257): 4 -> 2; tvd (E = 10 x 257, ITM only): 3 -> 2
            executed -= 12 * (2 * 13 * 257 + 1 * 10 * 257) * 2 * 768 * 1536 * 3 / 1e12
    return nominal, executed


def compact_line(res):
    """The stdout line: the contract's fields verbatim + the numbers of every other object (their prose and per-variant tables stay in the full
    record on stderr)."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    out = {k: res[k] for k in keep}
    c = res["config"]
    out["config"] = {k: c[k] for k in ("workload", "per_gpu_batch", "global_batch", "frames_per_sample", "vision", "vit_layers", "parallelism",
                                       "droppath_schedule", "kept_branch_fraction", "optimizer_step_in_timed_region")}
    out["config"]["precision"] = c["precision"][:120]
    out["config"]["backward"] = c.get("backward")
    r = res.get("roofline")
    if r is not None:
        out["roofline"] = {k: r.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_unit", "launches", "avg_launch_ms",
                                                 "step_frac", "step_tflops", "executed_tflop_per_sample", "kept_branch_fraction")}
        out["roofline"]["all_gemm"] = r.get("all_gemm")
        if r.get("traffic_provenance"):
            out["roofline"]["traffic_provenance"] = r["traffic_provenance"][:60] + " ... (not measured in this run)"
    else:
        out["roofline"] = None
    cb = res.get("cpu_baseline")
    if cb is not None:
        out["cpu_baseline"] = dict(value=cb["value"], unit=cb["unit"], cores=cb["cores"], kind=cb["kind"], sample=cb["sample"][:230], cpu=cb.get("cpu"),
                                   host_threads=cb.get("host_threads"),
                                   anchors={k: round(v["samples_per_s"], 4) for k, v in (cb.get("anchors") or {}).items()})
    for k in ("samples_per_sec_per_gpu", "frames_per_sec_per_gpu", "step_mfma_frac", "peak_mem_gb", "peak_reserved_gb", "hbm_gb", "losses", "allocator"):
        out[k] = res.get(k)
    tp = res.get("tower_plan") or {}
    out["tower_plan"] = {k: tp.get(k) for k in ("frames", "frames_per_pass", "diet", "mlp_blocks_kept", "mlp_stash", "kept_fraction")}
    p = res.get("parity")
    if p is not None:
        worst = max(((k, v) for k, v in p.items() if isinstance(v, float) and k not in ("worst", "gate")), key=lambda kv: kv[1])
        out["parity"] = dict(worst=p["worst"], worst_tensor=worst[0], gate=p["gate"], tensors=sum(1 for v in p.values() if isinstance(v, float)) - 2,
                             metric="max|out - ref| / max|ref| vs reference fp32 CPU goldens, timed precision")
    sec = res.get("secondary")
    if sec is not None:
        out["secondary"] = {}
        for k, v in sec.items():
            if not isinstance(v, dict) or "error" in v:
                out["secondary"][k] = v
                continue
            e = {kk: v.get(kk) for kk in ("value", "unit", "ms_per_step", "steps", "per_gpu_batch", "step_mfma_frac", "peak_mem_gb") if v.get(kk) is not None}
            rr = v.get("roofline")
            if rr:
                e["all_gemm_tflops"] = (rr.get("all_gemm") or {}).get("tflops")
            out["secondary"][k] = e
    d = res.get("droppath_ab")
    if d is not None:
        out["droppath_ab"] = d if "error" in d else dict(speedup=d["speedup"], dense_value=d["dense_reference_schedule"]["value"], unit=d["unit"])
    pc = res.get("parity_config")
    if pc is not None:
        out["parity_config"] = pc if "error" in pc else dict(precision=pc["precision"][:60], value=pc["value"], ms_per_step=pc["ms_per_step"],
                                                             parity_worst=(pc.get("parity") or {}).get("worst"))
    op = res.get("other_precisions")
    if op is not None:
        out["other_precisions"] = {k: (v if "error" in v else dict(value=v["value"], ms_per_step=v["ms_per_step"], parity_worst=(v.get("parity") or {}).get("worst")))
                                   for k, v in op.items()}
    cm = res.get("comm")
    if cm is not None:
        out["comm"] = {k: cm[k] for k in ("error", "backend", "rccl_ranks", "world_size", "packed_allgather_us", "grad_bytes", "grad_reduce_exposed_ms_per_step",
                                          "per_rank_samples_per_s", "per_rank_exposed_reduce_ms", "forced_at_world_size_1", "ms_per_step_with_collectives",
                                          "ms_per_step_headline") if k in cm}
    out["full_record"] = "stderr line BENCH_FULL_JSON (per-variant GEMM table, parity per tensor, tower plans, notes)"
    return out


def main():
    args = parse()
    wl = WORKLOADS[args.workload]
    args.task = args.task or wl["task"]
    if "dtype" in wl and "--dtype" not in " ".join(sys.argv):
        args.dtype = wl["dtype"]
    if "batch" in wl and "--batch" not in " ".join(sys.argv):
        args.batch = wl["batch"]
    if "vision" in wl and "--vision" not in " ".join(sys.argv):
        args.vision = wl["vision"]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args)
    # The contract is ONE JSON line on stdout.  Libraries print there too (RCCL writes a version banner to the C-level stdout when its first
    # communicator comes up, flushed at exit - i.e. AFTER the JSON line): keep the real stdout aside, point fd 1 at stderr for the whole run
    # and write the line to the saved descriptor at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} (or without torchrun)")
    if ONE_DEVICE:
        local_rank = 0
    if torch.cuda.device_count() <= local_rank:
        sys.exit(f"bench.py: rank {rank} has no GPU (LOCAL_RANK {local_rank}, {torch.cuda.device_count()} visible)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if BACKEND == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(BACKEND)

    from mico_amd import runtime, ops
    from mico_amd.model import MiCo, default_cfg
    from mico_amd.weights import synth_state_dict, synth_inputs
    from mico_amd.distributed import GradBucketReducer, packed_all_gather

    set_precision(args.dtype)
    runtime.set_activation_diet(args.diet, args.diet_mlp_blocks)
    torch.manual_seed(rank)     # host RNG: stochastic-depth draws differ per rank (weights/inputs come from counter hashes)
    from mico_amd.functional import DropPlan
    DropPlan.skip_dropped = not args.dense_droppath
    cfg = default_cfg(args.vision, vision_layers=args.layers)
    model, sd_cpu = build_model(cfg, seed=0)
    if args.no_bert_dropout:
        model.multimodal_encoder.bert.config.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model.to(dev)
    model.eval() if args.eval_mode else model.train()
    b = args.batch
    state = dict(reducer=GradBucketReducer(model.parameters()) if world > 1 else None)
    optimizer = None
    if args.optimizer:
        from mico_amd.optim import AdamW
        decay = [p for n, p in model.named_parameters() if not any(k in n for k in ("bias", "LayerNorm.bias", "LayerNorm.weight"))]
        nodecay = [p for n, p in model.named_parameters() if any(k in n for k in ("bias", "LayerNorm.bias", "LayerNorm.weight"))]
        optimizer = AdamW([dict(params=decay, weight_decay=0.01, lr=1e-6), dict(params=nodecay, weight_decay=0.0, lr=1e-6)],
                          lr=1e-6, betas=(0.9, 0.98))
    finish_ms = []
    main_model = model

    def step(the_batch, task, model=model):
        # (optimizer and reducer belong to the main model: a secondary model - configs[1]'s ViT-B/16 - steps without them)
        mine = model is main_model
        model.zero_grad(set_to_none=True)
        losses = model(dict(the_batch), task, compute_loss=True, backward_scale=None if args.direct_backward else 1.0)
        total = sum(losses.values())
        total.backward()
        if state["reducer"] is not None and mine:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            state["reducer"].finish()
            e1.record()
            finish_ms.append((e0, e1))
        if optimizer is not None and mine:
            optimizer.step()
        return losses

    def timed_steps(n, the_batch, task, model=model):
        """EXACTLY n steps bracketed by barrier + synchronize on both sides; max over ranks."""
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            losses = step(the_batch, task, model)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = t.item()
        return el, losses

    def measure(wname, task, nb, steps, warmup, seed, detail=False, model=model):
        """One workload, timed: `warmup` untimed steps, then exactly `steps` timed ones with the per-launch GEMM timer on.  Returns the
        figures of a bench line for it (value, ms per step, executed TFLOP, MFMA fraction of the step, GEMM roofline, peak memory,
        the tower plan it ran under)."""
        w = WORKLOADS[wname]
        batch = {k: v.to(dev) for k, v in synth_inputs(dict(b=nb, **w["shape"]), seed=seed + rank).items()}
        for _ in range(warmup):
            step(batch, task, model)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        timer = None if args.no_gemm_timer else ops.KernelTimer()
        ops.GEMM_TIMER = timer
        DropPlan.stats[:] = [0, 0]
        finish_ms.clear()
        ms0 = torch.cuda.memory_stats()
        el, losses = timed_steps(steps, batch, task, model)
        ms1 = torch.cuda.memory_stats()
        ops.GEMM_TIMER = None
        kept = DropPlan.stats[0] / DropPlan.stats[1] if DropPlan.stats[1] else 1.0
        value = nb * world * steps / el
        nominal, executed = executed_tflop_per_sample(wname, task, kept, runtime.CFG.share_cross_kv, args.eval_mode)
        full = args.layers is None and model.config.vision_encoder_type == w.get("vision", "evaclip01_giant") and task == w["task"]
        step_tflops = executed * value / world if (full and executed) else None
        roofline = None
        if timer is not None and timer.records:
            if detail and rank == 0:
                gemm_detail_table(timer, steps)
            summ = timer.summary()
            per_variant = {kname(k): dict(launches=v["launches"], avg_ms=v["ms"] / v["launches"], tflops=v["flops"] / v["ms"] / 1e9)
                           for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"])}
            tot_flops = sum(v["flops"] for v in summ.values())
            tot_ms = sum(v["ms"] for v in summ.values())
            dom = max(summ.items(), key=lambda kv: kv[1]["ms"])
            achieved = dom[1]["flops"] / dom[1]["ms"] / 1e9
            peak = 5000.0 if dom[0][2] == 4 else MFMA_PEAK_TFLOPS     # dense MX-fp8 peak (MI355X_MICROARCH.md) for the fp8 kernel
            roofline = dict(bound="mfma", kernel=kname(dom[0]), achieved=achieved, peak=peak, unit="TFLOP/s", frac=achieved / peak,
                            traffic=None, launches=dom[1]["launches"], avg_launch_ms=dom[1]["ms"] / dom[1]["launches"],
                            all_gemm=dict(tflops=tot_flops / tot_ms / 1e9, share_of_step_time=tot_ms / 1e3 / el), variants=per_variant,
                            _dom=dom[0])
        res = dict(value=value, unit="samples/s", ms_per_step=el / steps * 1e3, steps=steps, warmup=warmup, per_gpu_batch=nb,
                   frames_per_sample=w["frames"], frames_per_sec=value * w["frames"], task=task, kept_branch_fraction=kept,
                   tflop_per_sample={"dense_nominal": nominal, "executed": executed}, step_executed_tflops_per_gpu=step_tflops,
                   step_mfma_frac=(step_tflops / MFMA_PEAK_TFLOPS) if step_tflops else None,
                   peak_mem_gb=torch.cuda.max_memory_allocated() / 2 ** 30, peak_reserved_gb=torch.cuda.max_memory_reserved() / 2 ** 30,
                   # caching-allocator events inside the timed region: a retry = a failed hipMalloc answered by releasing cached blocks (a device
                   # synchronisation each) - the price of running close to the HBM capacity; device mallocs = segments newly requested from the driver
                   allocator=dict(alloc_retries=ms1.get("num_alloc_retries", 0) - ms0.get("num_alloc_retries", 0),
                                  device_mallocs=ms1.get("num_device_alloc", 0) - ms0.get("num_device_alloc", 0),
                                  device_frees=ms1.get("num_device_free", 0) - ms0.get("num_device_free", 0)),
                   tower_plan=runtime.last_tower_plan,
                   losses={k: float(v.detach()) for k, v in losses.items()}, roofline=roofline)
        return res, batch

    def gemm_detail_table(timer, steps):
        tab = {}
        for (var, flops, e0, e1), det in zip(timer.records, timer.detail):
            d = tab.setdefault((var, det[1], det[2], det[3], det[4]), [0, 0.0, 0.0, 0])
            d[0] += 1; d[1] += flops; d[2] += e0.elapsed_time(e1); d[3] += det[0]
        print(f"{'(ta,tb,kernel)':>14s} {'N':>6s} {'K':>6s} {'epilogue':>10s} {'split':>5s} {'launches':>8s} {'avg M':>8s} {'avg us':>8s} {'TFLOP/s':>8s} {'ms/step':>8s}", file=sys.stderr)
        for key, d in sorted(tab.items(), key=lambda kv: -kv[1][2]):
            print(f"{str(key[0]):>14s} {key[1]:6d} {key[2]:6d} {key[3]:>10s} {key[4]:5d} {d[0]:8d} {d[3] / d[0]:8.0f} {d[2] / d[0] * 1e3:8.1f} "
                  f"{d[1] / d[2] / 1e9:8.1f} {d[2] / steps:8.2f}", file=sys.stderr)

    # ================= the headline measurement =================
    head, batch = measure(args.workload, args.task, b, args.steps, args.warmup, seed=1234, detail=args.gemm_detail)
    elapsed = head["ms_per_step"] * args.steps / 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, head["losses"])

    # ---- communication figures: exposed gradient-reduction wait per step, packed all-gather latency.  N > 1: from the timed steps.
    # N = 1: the SAME code on a one-rank RCCL group (mico_amd.distributed.force_dist: packed_all_gather's all_gather_into_tensor,
    # fetch_rows' all_to_all_single, the reducer's in-place all_reduce(AVG) of the tower's arena slices + its buckets), a few extra steps
    # after the headline measurement - what a 1-GPU box can say about the N > 1 path: that it runs on RCCL and what its overhead is.
    comm = None
    forced_ms = None
    forced_peak = None
    exposed = sum(e0.elapsed_time(e1) for e0, e1 in finish_ms) / max(1, len(finish_ms)) if finish_ms else None
    if args.full and world == 1 and not args.no_comm and rank == 0:
        from mico_amd import distributed as D
        try:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
            D.force_dist(True)
            # the reducer's buckets (one fp32 copy of the gradients) change the tower plan: start from an empty allocator cache and give the new plan two
            # untimed steps, as a rank of an N > 1 job gets from its warm-up (with the headline's cached blocks in place the first steps of the new
            # plan free and re-request device memory: 1742 ms per step measured that way against 1512)
            release_memory()
            state["reducer"] = GradBucketReducer(model.parameters())
            step(batch, args.task)
            step(batch, args.task)
            finish_ms.clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            kc = max(2, args.steps // 4)
            elc, _ = timed_steps(kc, batch, args.task)
            forced_ms = elc / kc * 1e3
            forced_peak = torch.cuda.max_memory_allocated() / 2 ** 30
            exposed = sum(e0.elapsed_time(e1) for e0, e1 in finish_ms) / max(1, len(finish_ms))
        except Exception as e:
            comm = {"error": repr(e)}
    if args.full and (world > 1 or forced_ms is not None) and comm is None:
        feat = torch.randn(b, 512, device=dev)
        ids = batch["input_ids"]
        for _ in range(3):
            packed_all_gather([feat, ids, batch["attention_mask"], feat])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            packed_all_gather([feat, ids, batch["attention_mask"], feat])
        torch.cuda.synchronize()
        ag_us = (time.perf_counter() - t0) / 20 * 1e6
        grad_bytes = sum(p.numel() for p in model.parameters() if p.requires_grad) * 4
        comm = dict(backend="nccl (RCCL)" if dist.get_backend() == "nccl" else dist.get_backend() + " (test switch MICO_BENCH_BACKEND: not an RCCL measurement)",
                    rccl_ranks=dist.get_world_size() if dist.get_backend() == "nccl" else 0, world_size=dist.get_world_size(), packed_allgather_us=ag_us,
                    packed_allgather_bytes_per_rank=int(feat.numel() * 4 * 2 + ids.numel() * 8 * 2),
                    grad_bytes=grad_bytes, grad_reduce_exposed_ms_per_step=exposed,
                    grad_reduce_note="time the step spends in GradBucketReducer.finish() waiting for reductions that did not hide behind "
                                     "the backward; the ViT blocks' arena slices are reduced in place from inside the backward")
        if world > 1:
            # per-rank throughput of the timed region (the headline divides the global sample count by the MAX over ranks): a rank far
            # below the others, or an exposed reduction that grows with N, shows here without another run
            mine = torch.tensor([b * args.steps / elapsed, exposed or 0.0], device=dev, dtype=torch.float64)
            allr = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allr, mine)
            comm["per_rank_samples_per_s"] = [float(t[0]) for t in allr]
            comm["per_rank_exposed_reduce_ms"] = [float(t[1]) for t in allr]
        if forced_ms is not None:
            comm.update(forced_at_world_size_1=True, ms_per_step_with_collectives=forced_ms, steps=kc, peak_mem_gb_with_collectives=forced_peak,
                        ms_per_step_headline=head["ms_per_step"],
                        note="one-rank RCCL group with the N > 1 code paths forced (MICO_FORCE_DIST semantics): every collective of the "
                             "data-parallel step executes on RCCL, the reducer's buckets are allocated; latencies are one-rank figures, "
                             "not xGMI figures")
    if world == 1 and dist.is_initialized():
        from mico_amd import distributed as D
        D.force_dist(False)
        if state["reducer"] is not None:
            state["reducer"].close()
        state["reducer"] = None
        dist.destroy_process_group()
    if rank != 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # HBM bytes per launch of the dominant kernel: PMC counters cannot be read from inside this process; they come from the separate
    # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same command (profiles/*_gemm_hbm_traffic.json, FETCH_SIZE doubled as
    # MI355X_MICROARCH.md prescribes for gfx950).  null when no such profile is present.
    roofline = head.pop("roofline")
    if roofline is not None:
        dom = roofline.pop("_dom")
        for tname in ("r06_gemm_hbm_traffic.json", "r05_gemm_hbm_traffic.json", "r04_gemm_hbm_traffic.json", "r03_gemm_hbm_traffic.json", "r02_gemm_hbm_traffic.json"):
            tpath = os.path.join(ROOT, "profiles", tname)
            if os.path.exists(tpath) and world == 1:
                tj = json.load(open(tpath))
                key = {(0, 0): "NN", (0, 1): "dX", (1, 1): "dW", (1, 0): "TN"}[dom[:2]] + "_" + {0: "small", 1: "big", 2: "pc", 3: "w4", 4: "mx8", 5: "big", 6: "mid", 7: "mid", 8: "p8"}[dom[2]]
                if key in tj:
                    roofline["traffic"] = tj[key]["hbm_bytes_per_launch"]
                    roofline["traffic_unit"] = "bytes/launch"
                    roofline["traffic_provenance"] = (f"profiles/{tname}: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over bench.py on the builder's "
                                                      "box (tools/profile_round.sh; FETCH_SIZE doubled for gfx950) - PMC counters cannot be read from inside "
                                                      "this process, so this figure is NOT measured in this run")
                    break

    if roofline is not None:
        # the STEP next to the dominant kernel (the driver keeps this object): executed algorithmic TFLOP/s of the whole fwd+bwd
        # step over the dense 16-bit MFMA peak, what was executed per sample, the kept stochastic-depth fraction, all GEMM launches together
        roofline["step_frac"] = head["step_mfma_frac"]
        roofline["step_tflops"] = head["step_executed_tflops_per_gpu"]
        roofline["executed_tflop_per_sample"] = (head["tflop_per_sample"] or {}).get("executed")
        roofline["kept_branch_fraction"] = head["kept_branch_fraction"]
    res = {
        "metric": "omni-modal samples/sec (ViT-g/14 fwd+bwd)", "value": head["value"], "unit": "samples/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": args.dtype.split("-")[0], "data": "synthetic",
        "config": {"workload": WORKLOAD_TEXT[args.workload].format(b=b, task=args.task),
                   "per_gpu_batch": b, "global_batch": b * world, "frames_per_sample": wl["frames"], "precision": PRECISIONS[args.dtype][3],
                   "vision": args.vision, "vit_layers": args.layers or "full", "parallelism": f"dp{world}",
                   "droppath": ("off (eval)" if args.eval_mode else "on, reference rates (0 -> 0.4 linear)"),
                   "droppath_schedule": ("dense: every branch evaluated then scaled by 0 | 1/keep" if args.dense_droppath
                                         else "dropped (block, branch, frame) triples are skipped - exact, zero contribution"),
                   "backward": ("direct: one backward over every graph of the step" if args.direct_backward else
                                "staged: BERT passes differentiated one condition set at a time inside the forward (MiCo.forward(backward_scale=1.0)), "
                                "towers in the caller's backward - same values and gradients"),
                   "kept_branch_fraction": head["kept_branch_fraction"], "optimizer_step_in_timed_region": bool(args.optimizer),
                   "bert_dropout": (False if (args.eval_mode or args.no_bert_dropout) else
                                    "on: p=0.1 hidden + attention-probability (reference config.json)")},
        "samples_per_sec_per_gpu": head["value"] / world,
        "frames_per_sec_per_gpu": head["frames_per_sec"] / world,
        "step_executed_tflops_per_gpu": head["step_executed_tflops_per_gpu"],
        "tflop_per_sample": head["tflop_per_sample"],
        "cross_kv": "condition K/V projected once per step and shared by the ITM triplet and the captioning pass" if runtime.CFG.share_cross_kv else "per pass",
        "step_mfma_frac": head["step_mfma_frac"],
        "losses": head["losses"],
        "peak_mem_gb": head["peak_mem_gb"],
        "peak_reserved_gb": head["peak_reserved_gb"],
        "allocator": head["allocator"],
        "hbm_gb": torch.cuda.get_device_properties(dev).total_memory / 2 ** 30,
        "tower_plan": head["tower_plan"],
        "roofline": roofline,
    }
    if comm is not None:
        res["comm"] = comm
    extras = args.full and not args.no_extras and args.workload in ("omni", "img_aud_txt") and not args.optimizer
    if extras:
        # ---- the timed precision against the reference goldens, measured here and now ----
        del batch
        release_memory()
        # (rank 0 alone from here on - the other ranks wait at the final barrier: its alignment steps must not enter collectives)
        from mico_amd.distributed import local_only
        with local_only():
            res["parity"] = dict(precision=PRECISIONS[args.dtype][3], **measure_parity(model, dev))
    if extras and world == 1:
        # ---- the other ViT-g/14 configuration of BASELINE.json, timed as a first-class object next to the headline: configs[2] (image +
        # audio + text, 5 frames per sample: the headline of rounds 1-3) when the headline is the omni share, and vice versa
        other = "img_aud_txt" if args.workload == "omni" else "omni"
        try:
            release_memory()
            sec, sbatch = measure(other, WORKLOADS[other]["task"], b, max(10, args.steps // 2), 2, seed=4321)
            r2 = sec.get("roofline")
            if r2 is not None:
                r2.pop("_dom", None)
                r2.pop("variants", None)
            sec["precision"] = PRECISIONS[args.dtype][3]
            sec["workload"] = WORKLOAD_TEXT[other].format(b=b, task=WORKLOADS[other]["task"])
            res["secondary"] = {("configs2_img_aud_txt" if other == "img_aud_txt" else "omni_configs3_rank_share"): sec}
            del sbatch
            if args.dtype != "bf16":
                # BASELINE.json names configs[2] "bf16": the same step with bf16 MFMA operands, reported (not gated - bf16 keeps 8
                # mantissa bits; the gated 16-bit configuration is the fp16 one above)
                try:
                    set_precision("bf16")
                    release_memory()
                    sbf, bbf = measure("img_aud_txt", WORKLOADS["img_aud_txt"]["task"], b, max(5, args.steps // 4), 2, seed=4321)
                    del bbf
                    res["secondary"]["configs2_img_aud_txt_bf16"] = dict(value=sbf["value"], unit="samples/s", ms_per_step=sbf["ms_per_step"], steps=sbf["steps"],
                                                                         step_mfma_frac=sbf["step_mfma_frac"], peak_mem_gb=sbf["peak_mem_gb"],
                                                                         precision=PRECISIONS["bf16"][3])
                except Exception as e:
                    res["secondary"]["configs2_img_aud_txt_bf16"] = {"error": repr(e)}
                finally:
                    set_precision(args.dtype)
        except Exception as e:   # the headline line must survive a failure of the secondary measurement
            res["secondary"] = {"error": repr(e)}
        # ---- BASELINE configs[1] (ViT-B/16 image + text contrastive step, b = 256): its own model, timed with its own GEMM roofline ----
        if args.workload != "b16_img_txt":
            try:
                release_memory()
                wb = WORKLOADS["b16_img_txt"]
                mb = MiCo(default_cfg(wb["vision"]))
                mb.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in mb.state_dict().items()}, seed=0), strict=False)
                mb.to(dev)
                mb.eval() if args.eval_mode else mb.train()
                secb, bb = measure("b16_img_txt", wb["task"], wb["batch"], max(10, args.steps // 2), 3, seed=2468, model=mb)
                rb = secb.get("roofline")
                if rb is not None:
                    rb.pop("_dom", None)
                    rb.pop("variants", None)
                secb["precision"] = PRECISIONS[args.dtype][3] + " (EVA02-style towers: their head-split blocks run the 3-segment mode, DESIGN.md section 4)"
                secb["workload"] = WORKLOAD_TEXT["b16_img_txt"].format(b=wb["batch"], task=wb["task"])
                res.setdefault("secondary", {})["configs1_b16_img_txt"] = secb
                del bb, mb
            except Exception as e:
                res.setdefault("secondary", {})["configs1_b16_img_txt"] = {"error": repr(e)}
        # ---- what skipping the dropped stochastic-depth branches is worth: the same step on the reference's schedule (every branch
        # evaluated, dropped ones multiplied by 0) - identical values and gradients, more work, its own tower plan ----
        if not args.eval_mode and not args.dense_droppath:
            try:
                release_memory()
                DropPlan.skip_dropped = False
                kd = max(3, args.steps // 5)
                dm, db_ = measure(args.workload, args.task, b, kd, 1, seed=1234)
                del db_
                res["droppath_ab"] = dict(skipped_branches=dict(value=head["value"], ms_per_step=head["ms_per_step"], kept_branch_fraction=head["kept_branch_fraction"]),
                                          dense_reference_schedule=dict(value=dm["value"], ms_per_step=dm["ms_per_step"], steps=kd, warmup=1,
                                                                        peak_mem_gb=dm["peak_mem_gb"], tower_plan=dm["tower_plan"]),
                                          unit="samples/s", speedup=head["value"] / dm["value"],
                                          note="same step, same precision, same process; `dense` = bench.py --dense-droppath")
            except Exception as e:
                res["droppath_ab"] = {"error": repr(e)}
            finally:
                DropPlan.skip_dropped = True
        # ---- the same (headline) step in the configuration with margin under the 1e-3 gate, timed next to it ----
        release_memory()
        pc = "fp16-split-w" if args.dtype != "fp16-split-w" else "fp16"
        names = [pc] + ([oc for oc in ("fp16-plain", "fp8") if oc != args.dtype] if args.all_precisions else [])
        k2 = max(3, args.steps // 5)
        others = {}
        from mico_amd import functional as _Fn
        soft0 = _Fn._SOFT_FRAC
        for oc in names:
            try:
                set_precision(oc)
                release_memory()
                # a process that has already run five other measurements (and RCCL) carries their allocator history: the weights-split step planned
                # at the headline's soft budget reserved 277 GiB of the 288 here and paid for it in allocator retries (1 retry, 16 device mallocs,
                # 126 frees inside 3 timed steps: 2209 ms per step against 1792 in a process of its own) - these extras plan 0.04 lower
                _Fn._SOFT_FRAC = soft0 - 0.04
                m, pb = measure(args.workload, args.task, b, k2, 1, seed=1234)
                del pb
                entry = dict(precision=PRECISIONS[oc][3], value=m["value"], unit="samples/s", steps=k2, warmup=1, ms_per_step=m["ms_per_step"],
                             peak_mem_gb=m["peak_mem_gb"], peak_reserved_gb=m.get("peak_reserved_gb"), allocator=m.get("allocator"), tower_plan=m.get("tower_plan"),
                             hbm_soft_frac=_Fn._SOFT_FRAC, parity=measure_parity(model, dev))
                if oc == "fp8":
                    entry["parity_note"] = ("the golden inputs (1-8 frames) are below the size at which GEMMs route to the fp8 kernel (>= 128 "
                                            "tiles of 256x256): this parity is the bf16 path's; the fp8 tolerance is measured by "
                                            "tests/test_model_gpu.py::test_fp8_tower_tolerance and tests/test_full_size_gpu.py")
                others[oc] = entry
            except Exception as e:
                others[oc] = {"error": repr(e)}
            finally:
                _Fn._SOFT_FRAC = soft0
        set_precision(args.dtype)
        res["parity_config"] = others.pop(pc)
        if others:
            res["other_precisions"] = others
    if args.full and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(sd_cpu, args)
    sys.stdout.flush()
    # The complete record goes to stderr (and to MICO_BENCH_FULL, a path, when set: tools/profile_round.sh keeps it under profiles/); the ONE line on
    # stdout is its compact form - every contract field, `roofline` with the step-level figures, `cpu_baseline`, and the headline numbers of the
    # other objects - so that a tail of a few KB holds all of it (the round-5 line was > 8 KB and the driver's tail cut its head off).
    full = json.dumps(res)
    print("BENCH_FULL_JSON " + full, file=sys.stderr, flush=True)
    if os.environ.get("MICO_BENCH_FULL"):
        with open(os.environ["MICO_BENCH_FULL"], "w") as fh:
            fh.write(full + "\n")
    os.write(real_stdout, (json.dumps(compact_line(res)) + "\n").encode())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
