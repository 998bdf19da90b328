#!/usr/bin/env python
"""inference_demo.py - the reference's demo entry point (inference_demo.py:14-174) on the MI355X path.

    python inference_demo.py --pretrain_dir MiCo-g --image example/test.jpeg            # a real checkpoint directory
    python inference_demo.py --synthetic evaclip01_giant --image some.jpeg               # no checkpoint: synthetic weights

`load_from_pretrained_dir(pretrain_dir, video_resolution, return_modal) -> (checkpoint, model_cfg)` keeps the reference's
contract: reads log/hps.json, picks ckpt/model_step_<max>.pt, renames video->vision / evaclip_model|clip_model->vision_encoder,
casts to fp32, nearest-interpolates the frame embeddings to max_*_sample_num and bilinearly interpolates the ViT position
table to the requested resolution.  The demo then encodes the image and the texts, prints the text-to-image similarity, the ITM
scores and a beam-search caption (BertForMaskedLM.generate, :161-174).

    python inference_demo.py --synthetic evaclip01_giant --image some.jpeg --audio clip.wav   # + the audio-text similarity [1, texts]

--audio FILE.wav: the clip goes from the file to the tower's windows on the device (AudioProcessor: PCM decode, resample to 16 kHz, Kaldi
log-mel filterbank, normalise / window) and its similarity to every text is printed after the image's lines, through the encoder, pooling
and heads of the ret%ta sub-task.

--transforms {none,crop_flip}: the reference's --vision_transforms, passed to the image processor and to the video processor of --video.  The
demo runs in evaluation mode, so crop_flip is Resize(224) + CenterCrop(224) (the shorter side goes to 224, the central window is kept) instead
of `none`'s Resize((224, 224)).

--video FOLDER: a folder of extracted frames goes through VideoProcessor (max_vision_sample_num frames, decoded on the host, transformed on the
device) and its similarity to every text is printed after the image's lines.
"""
import argparse
import json
import os
from collections import defaultdict

import torch
import torch.nn.functional as F

from mico_amd.model import MiCo, AttrDict, default_cfg


def load_from_pretrained_dir(pretrain_dir, video_resolution=224, return_modal="full"):
    checkpoint_dir = os.path.join(pretrain_dir, "ckpt")
    file_cfg = json.load(open(os.path.join(pretrain_dir, "log", "hps.json")))
    model_cfg = AttrDict(file_cfg["model_cfg"])
    steps = sorted(int(i.split("_")[2].split(".")[0]) for i in os.listdir(checkpoint_dir) if i.startswith("model_step"))
    ckpt_file = os.path.join(checkpoint_dir, f"model_step_{steps[-1]}.pt")
    checkpoint = torch.load(ckpt_file, map_location="cpu")
    print(f"load_from_pretrained: {ckpt_file}")
    new_ckpt = {}
    for k, v in checkpoint.items():
        if "video" in k:
            new_ckpt[k.replace("video", "vision")] = v
        elif "evaclip_model" in k:
            new_ckpt[k.replace("evaclip_model", "vision_encoder")] = v
        elif "clip_model" in k:
            new_ckpt[k.replace("clip_model", "vision_encoder")] = v
        else:
            new_ckpt[k] = v.float()
    checkpoint = new_ckpt
    if model_cfg.frame_embedding_type == "adaptive":
        vkey = "vision_frame_embedding" if "vision_frame_embedding" in checkpoint else "vision_perceiver.vision_frame_embedding"
        wanted = [(vkey, model_cfg.max_vision_sample_num)]      # a checkpoint with neither vision key is a KeyError, as upstream
        if "audio_frame_embedding" in checkpoint:
            wanted.append(("audio_frame_embedding", model_cfg.max_audio_sample_num))
        for key, n in wanted:
            emb = checkpoint[key]
            if emb.shape[1] != n:
                checkpoint[key] = F.interpolate(emb.permute(0, 2, 1), n, mode="nearest").permute(0, 2, 1)
    vtype = model_cfg.vision_encoder_type
    if vtype.startswith("clip") or vtype.startswith("evaclip"):
        # OpenAI-CLIP towers keep a 2-D table, EVA towers a [1, 1+g*g, D] one; both resize the patch part bilinearly
        eva = vtype.startswith("evaclip")
        pk = "vision_encoder.visual.pos_embed" if eva else "vision_encoder.visual.positional_embedding"
        wk = "vision_encoder.visual.patch_embed.proj.weight" if eva else "vision_encoder.visual.conv1.weight"
        table = checkpoint[pk][0] if eva else checkpoint[pk]
        width, patch = table.shape[-1], checkpoint[wk].shape[-1]
        grid = round((table.shape[0] - 1) ** 0.5)
        new_grid = model_cfg.vision_resolution // patch
        if new_grid != grid:
            oth = table[1:].reshape(grid, grid, width).permute(2, 0, 1).unsqueeze(0)
            oth = F.interpolate(oth, (new_grid, new_grid), mode="bilinear")[0].permute(1, 2, 0).reshape(-1, width)
            table = torch.cat((table[0:1], oth), dim=0)
            checkpoint[pk] = table.unsqueeze(0) if eva else table
    if return_modal == "uni":
        out = defaultdict()
        for k in checkpoint:
            if "video_encoder" in k:
                out[".".join(k.split(".")[1:])] = checkpoint[k]
        checkpoint = out
    elif return_modal == "text":
        out = defaultdict()
        for k in checkpoint:
            if "multimodal_encoder" in k:
                out[".".join(k.split(".")[1:])] = checkpoint[k]
        checkpoint = out
    return checkpoint, model_cfg


def write_synthetic_pretrain_dir(path, vision_encoder_type="evaclip01_giant", steps=(5, 10), seed=0, **cfg_over):
    """A stand-in for the released `MiCo-g/` directory (no network here): hps.json + ckpt/model_step_<n>.pt with synthetic
    weights stored under the *pre-rename* key names a released checkpoint uses, so the loader's remap path is exercised."""
    from mico_amd.weights import synth_state_dict
    cfg = default_cfg(vision_encoder_type, **cfg_over)
    os.makedirs(os.path.join(path, "ckpt"), exist_ok=True)
    os.makedirs(os.path.join(path, "log"), exist_ok=True)
    json.dump({"model_cfg": dict(cfg)}, open(os.path.join(path, "log", "hps.json"), "w"))
    m = MiCo(cfg)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    stored = {}
    for k, v in sd.items():
        k2 = k.replace("vision_encoder", "evaclip_model") if k.startswith("vision_encoder") else k.replace("vision_", "video_")
        stored[k2] = v.clone()
    for s in steps:
        torch.save(stored if s == max(steps) else {}, os.path.join(path, "ckpt", f"model_step_{s}.pt"))
    return cfg, sd


@torch.no_grad()
def run_demo(model, image_input, texts, device="cuda", max_length=30, use_cache=False, rerank=False, questions=None, device_search=False,
             no_repeat_ngram_size=0, repetition_penalty=1.0, sample_captions=0, top_k=10, top_p=1.0, temperature=1.0):
    """The retrieval + matching part of the reference's __main__ (inference_demo.py:128-158).  use_cache: the caption's beam search
    decodes incrementally (BertForMaskedLM.generate(use_cache=True)).  rerank: the ITM scores come from the retrieval evaluation path
    (mico_amd.evaluation.rerank_retrieval: the image's condition tokens projected once, every text reading them by index) instead of one
    copy of the tokens per text - the same scores.  questions (list[str]; None: none asked): the image's answers to them
    (MiCo.forward_qa, vast.py:557-650) as "answers" - with use_cache the image's condition tokens are projected once for all questions.
    device_search: the caption's and the answers' beam search runs on the device (generate(device_search=True)); no_repeat_ngram_size /
    repetition_penalty: generate()'s logits processors for both (0 / 1.0: off).
    sample_captions N > 0: also N sampled captions of the image as "sampled_captions" (BertForMaskedLM.sample on the device: top_k, top_p,
    temperature, and the two processors above)."""
    image_input = image_input.to(device).unsqueeze(1)          # image as a 1 frame video
    video_output = model.forward_vision_encoder(image_input)
    feat_v = F.normalize(model.contra_head_v(model.pool_vision_for_contra(video_output)), dim=-1)
    tok = model.multimodal_encoder.tokenizer(texts, padding="max_length", truncation=True, max_length=max_length, return_tensors="pt")
    input_ids, attention_mask = tok.input_ids.to(device), tok.attention_mask.to(device)
    caption_output = model.forward_multimodal_encoder(input_ids, attention_mask).sequence_output
    feat_t = F.normalize(model.contra_head_t(model.pool_text_for_contra(caption_output)), dim=-1)
    sim_t2v = torch.matmul(feat_t, feat_v.permute(1, 0))
    video_input = model.get_multimodal_forward_input_vision(video_output)
    if rerank:
        from mico_amd import runtime
        from mico_amd.evaluation import rerank_retrieval
        # every text's shortlist is the one image (k = 1): itm_scores [texts, 1] is the demo's score per text
        res = rerank_retrieval(model, feat_t, input_ids, attention_mask, feat_v, video_input.to(runtime.compute_dtype()), k=1,
                               directions=("t2c",))
        slice_scores = res["t2c"]["itm_scores"][:, 0]
    else:
        video_input = video_input.expand(input_ids.shape[0], -1, -1).contiguous()
        slice_output = model.forward_multimodal_encoder(input_ids, attention_mask, video_input).sequence_output
        slice_scores = F.softmax(model.itm_head(slice_output[:, 0]), dim=1)[:, 1]
    # caption generation (inference_demo.py:161-174)
    cap_input = model.get_multimodal_forward_input_vision(video_output)
    tk = model.multimodal_encoder.tokenizer
    init_ids = torch.full((cap_input.size(0), 1), tk.bos_token_id, dtype=torch.long, device=device)
    search = {}      # (only what is switched on is passed: the plain call stays the plain call)
    if device_search:
        search["device_search"] = True
    if int(no_repeat_ngram_size):
        search["no_repeat_ngram_size"] = int(no_repeat_ngram_size)
    if float(repetition_penalty) != 1.0:
        search["repetition_penalty"] = float(repetition_penalty)
    outputs = model.multimodal_encoder.generate(input_ids=init_ids, attention_mask=init_ids.new_ones(cap_input.size(0), 1, 1),
                                                encoder_hidden_states=cap_input, max_new_tokens=model.max_caption_len,
                                                num_beams=model.beam_size, eos_token_id=tk.sep_token_id,
                                                pad_token_id=tk.pad_token_id, length_penalty=0.6, use_cache=use_cache, **search)
    captions = tk.batch_decode(outputs[:, 1:], skip_special_tokens=True)
    out = dict(feat_v=feat_v, feat_t=feat_t, sim_t2v=sim_t2v, itm_scores=slice_scores, input_ids=input_ids,
               caption_ids=outputs, captions=captions)
    if int(sample_captions) > 0:
        proc = {k: v for k, v in search.items() if k != "device_search"}
        sampled = model.multimodal_encoder.sample(input_ids=init_ids, attention_mask=init_ids.new_ones(cap_input.size(0), 1, 1),
                                                  encoder_hidden_states=cap_input, max_new_tokens=model.max_caption_len, top_k=int(top_k),
                                                  top_p=float(top_p), temperature=float(temperature), eos_token_id=tk.sep_token_id,
                                                  pad_token_id=tk.pad_token_id, num_return_sequences=int(sample_captions), use_cache=use_cache,
                                                  **proc)
        out["sampled_captions"] = tk.batch_decode(sampled[:, 1:], skip_special_tokens=True)
    if questions:
        # every question is asked of the one image: one sample with len(questions) questions
        keys = {"decode_use_cache": bool(use_cache), **{f"decode_{k}": v for k, v in search.items()}}
        before = {k: model.config[k] for k in keys if k in model.config}
        model.config.update(keys)
        try:
            qa = model.forward_qa({"vision_pixels": image_input, "raw_questions": [list(questions)]}, "qa%tv", compute_loss=False)
        finally:
            for k in keys:
                model.config.pop(k, None)
            model.config.update(before)
        out["answers"] = qa["generated_answers_tv"]
    return out


@torch.no_grad()
def run_video_demo(model, video_input, texts, device="cuda", max_length=30):
    """video_input: the frames of one clip [n, 3, r, r] (VideoProcessor) -> video-to-text similarity [1, len(texts)], formed as run_demo
    forms the image's."""
    video_output = model.forward_vision_encoder(video_input.to(device).unsqueeze(0))
    feat_v = F.normalize(model.contra_head_v(model.pool_vision_for_contra(video_output)), dim=-1)
    tok = model.multimodal_encoder.tokenizer(texts, padding="max_length", truncation=True, max_length=max_length, return_tensors="pt")
    caption_output = model.forward_multimodal_encoder(tok.input_ids.to(device), tok.attention_mask.to(device)).sequence_output
    feat_t = F.normalize(model.contra_head_t(model.pool_text_for_contra(caption_output)), dim=-1)
    return dict(feat_v=feat_v, feat_t=feat_t, sim_v2t=torch.matmul(feat_v, feat_t.permute(1, 0)))


@torch.no_grad()
def run_audio_demo(model, audio_input, texts, device="cuda", max_length=30):
    """audio_input: the windows of one clip [sample_num, target_length, mel] (AudioProcessor) -> audio-to-text similarity [1, len(texts)]:
    the tower on the spectrogram windows, CLS pooling and contra_head_a against the text feature, as ret%ta forms them."""
    audio_output = model.forward_audio_encoder(audio_input.to(device).unsqueeze(0))
    feat_a = F.normalize(model.contra_head_a(model.pool_audio_for_contra(audio_output)), dim=-1)
    tok = model.multimodal_encoder.tokenizer(texts, padding="max_length", truncation=True, max_length=max_length, return_tensors="pt")
    caption_output = model.forward_multimodal_encoder(tok.input_ids.to(device), tok.attention_mask.to(device)).sequence_output
    feat_t = F.normalize(model.contra_head_t(model.pool_text_for_contra(caption_output)), dim=-1)
    return dict(feat_a=feat_a, feat_t=feat_t, sim_a2t=torch.matmul(feat_a, feat_t.permute(1, 0)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrain_dir", default="MiCo-g")
    ap.add_argument("--synthetic", default=None, help="vision_encoder_type: build a synthetic pretrain dir instead of reading one")
    ap.add_argument("--image", default="example/test.jpeg")
    ap.add_argument("--texts", nargs="*", default=["a man is skiing in a snowy day.", "it's a hot day"])
    ap.add_argument("--question", action="append", default=None, help="a question about the image (repeatable); the answers are printed")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--use_cache", action="store_true", help="decode the caption incrementally (K/V cache; same caption)")
    ap.add_argument("--device_search", action="store_true", help="run the beam search itself on the device (same caption)")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0, metavar="N", help="no n-gram of this size twice in a caption (0: off)")
    ap.add_argument("--repetition_penalty", type=float, default=1.0, metavar="P", help="penalty on tokens already in the caption (1: off)")
    ap.add_argument("--sample_captions", type=int, default=0, metavar="N", help="also print N sampled captions (sampling decode on the device)")
    ap.add_argument("--top_k", type=int, default=10, help="sampled captions: keep the K best tokens per step (0: off)")
    ap.add_argument("--top_p", type=float, default=1.0, help="sampled captions: nucleus mass (1: off)")
    ap.add_argument("--temperature", type=float, default=1.0, help="sampled captions: softmax temperature")
    ap.add_argument("--rerank", action="store_true", help="ITM scores through the retrieval evaluation path (indexed K/V memory; same scores)")
    ap.add_argument("--audio", default=None, help="a PCM .wav clip: its audio-to-text similarity [1, texts] is printed after the image's lines")
    ap.add_argument("--video", default=None, help="a folder of frames: its video-to-text similarity [1, texts] is printed after the image's lines")
    ap.add_argument("--transforms", default="none", choices=["none", "crop_flip"],
                    help="vision transforms of both processors (evaluation mode: crop_flip = resize the shorter side + centre crop)")
    args = ap.parse_args(argv)
    device = "cuda"
    from mico_amd import runtime
    from mico_amd.model.imageprocessor import ImageProcessor
    runtime.set_compute_dtype(torch.float16 if args.dtype == "fp16" else torch.bfloat16)
    if args.synthetic:
        import tempfile
        args.pretrain_dir = tempfile.mkdtemp(prefix="mico_synth_")
        write_synthetic_pretrain_dir(args.pretrain_dir, args.synthetic)
    checkpoint, opts = load_from_pretrained_dir(args.pretrain_dir, video_resolution=224, return_modal="full")
    model = MiCo.from_pretrained(opts, checkpoint).to(device).eval()
    # (training only matters to crop_flip, which the demo wants in its evaluation form; `none` is the same transform either way)
    proc = ImageProcessor(image_resolution=224, image_encoder_type="swin", image_transforms=args.transforms, training=args.transforms == "none")
    image_input = proc(args.image)
    if image_input is None:
        raise SystemExit(f"cannot read {args.image}")
    out = run_demo(model, image_input, args.texts, device, use_cache=args.use_cache, rerank=args.rerank, questions=args.question,
                   device_search=args.device_search, no_repeat_ngram_size=args.no_repeat_ngram_size, repetition_penalty=args.repetition_penalty,
                   sample_captions=args.sample_captions, top_k=args.top_k, top_p=args.top_p, temperature=args.temperature)
    print(out["sim_t2v"])
    print(out["itm_scores"])
    print(out["captions"])
    if args.sample_captions > 0:
        print(out["sampled_captions"])
    if args.question:
        print(out["answers"])
    if args.video:
        from mico_amd.model.videoprocessor import VideoProcessor
        vproc = VideoProcessor(video_resolution=224, video_encoder_type="swin", sample_num=opts.max_vision_sample_num,
                               video_transforms=args.transforms, training=False, device=device)
        video_input = vproc(args.video)
        if video_input is None:      # unreadable (printed by the processor) or missing
            raise SystemExit(f"cannot read {args.video}")
        print(run_video_demo(model, video_input, args.texts, device)["sim_v2t"])
    if args.audio:
        from mico_amd.model.audioprocessor import AudioProcessor
        aproc = AudioProcessor(melbins=224, target_length=224, sample_num=opts.max_audio_sample_num, resize_melbin_num=224, training=False,
                               device=device)
        audio_input = aproc(args.audio)
        if audio_input is None or not audio_input.is_cuda:      # unreadable (printed by the processor) or missing
            raise SystemExit(f"cannot read {args.audio}")
        print(run_audio_demo(model, audio_input, args.texts, device)["sim_a2t"])


if __name__ == "__main__":
    main()
