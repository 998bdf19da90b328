"""MiCo.forward(batch, task, compute_loss) - the omni-modal alignment step.

Specification: the VAST sibling's trainer-facing forward (data/model/vast.py:317-348), forward_ret (:383-464: ITC with
label smoothing 0.1 against the all-gathered global batch, ITM with in-batch hard negatives) and forward_cap (:485-512:
causal masked-caption LM), generalised with MiCo's depth heads (model/mico.py:390,392,402,406).  These functions become
methods of mico_amd.model.mico.MiCo.

Entry points: forward (direct, or _forward_staged; evaluation: _eval_ret / _eval_cap), forward_qa ("qa%...", vast.py:557-650), forward_scst,
encode_batch; task strings go through _parse_task, text through _tokenize.  One definition each: _itm_draw, _itm_loss, _cap_loss, _cls_prompt.

batch keys: vision_pixels [b,n,3,h,w] | audio_spectrograms [b,n,h,w] | depth_pixels [b,n,3,h,w] (any subset);
            raw_captions (list[str]) or input_ids/attention_mask [b,S].
            forward_qa: raw_questions (list[str]; evaluation: or list[list[str]]) / raw_answers, or question_ids / question_mask
            [nq, Lq] (+ num_questions, list[int], for several questions per sample) and answer_ids / answer_mask [b, La].
            optional `_injected`: {subtask: {neg_cond_idx, neg_text_idx}, "cap" / "qa": {masked_ids, labels}} replaces the RNG draws
            (torch.multinomial / TokenMasker) for parity tests, "drop_path_scale" / "patch_keep" ({modality: [depth, 2, b*n] /
            int [b*n, keep]}) the tower's stochastic-depth and patch-dropout draws; optional `_world`: simulated gathered tensors.
"""
import collections

import torch

from .. import distributed as D
from .. import functional as Fn, ops
from .. import runtime
from .bert import first_eos_valid

COND_MODALITY = {"v": "vision", "a": "audio", "d": "depth"}
FUSED_HEADS = {"v": "contra_head_v", "a": "contra_head_a", "d": "contra_head_d", "s": "contra_head_s", "va": "contra_head_va",
               "vd": "contra_head_id", "vs": "contra_head_vs", "vas": "contra_head_vas"}
_UNKNOWN_FAMILY = "{}: MiCo.forward runs the ret% / itc% / cap% families; question answering (qa%...) is MiCo.forward_qa"
SUBTASKS = ("tv", "ta", "td", "ts", "tva", "tvd", "tvs", "tvas")    # vast.py's tv / ta / tva / tvs / tvas + MiCo's depth heads
_FAMILIES = {"forward": ("ret", "itc", "cap"), "forward_qa": ("qa",), "forward_scst": ("cap",)}


def _parse_task(task, entry):
    """[(family, [sub-task, ...]), ...] of a task string like "ret%tva%tv_cap%tva" for the entry point `entry` (a key of _FAMILIES).  forward
    takes any number of its families and raises NotImplementedError for another one; forward_qa and forward_scst take exactly one family with
    at least one sub-task and raise ValueError otherwise.  A sub-task outside SUBTASKS is a ValueError for all of them."""
    parts, parsed = str(task).split("_"), []
    for t in parts:
        kind, *subtasks = t.split("%")
        if entry == "forward":
            if kind not in _FAMILIES[entry]:
                raise NotImplementedError(_UNKNOWN_FAMILY.format(t))
        elif kind not in _FAMILIES[entry] or not subtasks or len(parts) > 1:
            raise ValueError(f"{entry}: task {task!r} is not of the form {_FAMILIES[entry][0]}%<sub-task>%...")
        for st in subtasks:
            if st not in SUBTASKS:
                raise ValueError(f"{entry}: unknown sub-task {st!r} in {task!r}")
        parsed.append((kind, subtasks))
    return parsed


def _tokenize(self, texts, max_length):
    """token ids and key-padding mask [len(texts), max_length] from the BERT tokenizer, on the model's device"""
    dev = self.contra_temp.device
    tok = self.multimodal_encoder.tokenizer(texts, padding="max_length", truncation=True, max_length=max_length, return_tensors="pt")
    return tok.input_ids.to(dev), tok.attention_mask.to(dev)


def _tokens(self, batch):
    if "input_ids" in batch:
        return batch["input_ids"], batch["attention_mask"]
    if "caption_tokens" in batch:
        ct = batch["caption_tokens"]
        return ct.input_ids, ct.attention_mask
    batch["input_ids"], batch["attention_mask"] = _tokenize(self, batch["raw_captions"], self.max_caption_len)
    return batch["input_ids"], batch["attention_mask"]


def encode_batch(self, batch):
    """batch_get of vast.py:81-314 for every modality present: ONE tower pass over all frames of all modalities (they share
    the ViT), pooled features, packed condition tensors, text feature."""
    enc = {}
    groups, meta = [], []
    for m, key in (("v", "vision_pixels"), ("a", "audio_spectrograms"), ("d", "depth_pixels")):
        if key not in batch:
            continue
        x = batch[key]
        b, n = x.shape[:2]
        g = x.reshape(b * n, 1, *x.shape[-2:]) if m == "a" else x.reshape(b * n, *x.shape[2:])
        groups.append(g)
        meta.append((m, b, n))
    if groups:
        # injected stochastic-depth multipliers ({modality: [depth, 2, b*n]}; parity tests) are laid out like the frames
        dps = (batch.get("_injected") or {}).get("drop_path_scale")
        if dps is not None:
            dps = torch.cat([dps[m].float().cpu() for m, _, _ in meta], dim=-1)
        # injected patch-dropout tables ({modality: int [b*n, keep]}), concatenated in the same frame order; otherwise the tower draws ONE
        # table over all frames of the pass
        pk = (batch.get("_injected") or {}).get("patch_keep")
        if pk is not None:
            pk = torch.cat([torch.as_tensor(pk[m]).cpu() for m, _, _ in meta], dim=0)
        if self.config.vision_encoder_type.startswith("swin"):
            if pk is not None:
                raise ValueError("patch_keep was injected but the Swin tower has no patch dropout")
            # one tower pass as well; spectrograms take the reference's route of three identical channels (mico.py:139-140)
            frames = torch.cat([g.expand(-1, 3, -1, -1) if g.shape[1] == 1 else g for g in groups], dim=0)
            tokens = self.vision_encoder.forward_features(frames, drop_path_scale=dps)
        else:
            tokens = self.vision_encoder.visual.forward_groups(groups, drop_path_scale=dps, patch_keep=pk)
        f0 = 0
        for m, b, n in meta:
            o = tokens[f0:f0 + b * n].view(b, n, *tokens.shape[-2:])
            f0 += b * n
            enc["output_" + m] = o
            enc["pooled_" + m] = self.pool_vision_for_contra(o)
            enc["condition_feats_" + m] = self._pack(COND_MODALITY[m], o)
    if "subtitle_ids" in batch or "raw_subtitles" in batch:   # vast.py:96-104,168-174: subtitles through the text BERT
        if "subtitle_ids" not in batch:
            batch["subtitle_ids"], batch["subtitle_mask"] = _tokenize(self, batch["raw_subtitles"], self.max_subtitle_len)
        sub = self.multimodal_encoder.bert(input_ids=batch["subtitle_ids"], attention_mask=batch["subtitle_mask"]).last_hidden_state
        enc["output_s"] = sub
        enc["pooled_s"] = self.pool_text_for_contra(sub)
        enc["condition_feats_s"] = self.get_multimodal_forward_input_subtitle(sub)
    if "input_ids" in batch or "raw_captions" in batch or "caption_tokens" in batch:
        ids, am = _tokens(self, batch)
        seq = self.multimodal_encoder.bert(input_ids=ids, attention_mask=am).last_hidden_state
        enc["caption_output"] = seq
        enc["feat_t"] = Fn.l2_normalize(self.contra_head_t(self.pool_text_for_contra(seq)))
    return enc


def _feat_cond(self, enc, cond):
    pooled = torch.cat([enc["pooled_" + m] for m in cond], dim=1) if len(cond) > 1 else enc["pooled_" + cond]
    return Fn.l2_normalize(getattr(self, FUSED_HEADS[cond])(pooled))


def _condition_feats(self, enc, cond):
    if len(cond) == 1:
        return enc["condition_feats_" + cond]
    return torch.cat([enc["condition_feats_" + m] for m in cond], dim=1)


def _share_cross_kv(self):
    """Share the cross-attention K/V projections between the passes of a training step (runtime.CFG.share_cross_kv)."""
    return runtime.CFG.share_cross_kv and torch.is_grad_enabled()


# What the ITM hard-negative draw of one sub-task leaves for its triplet pass: neg_c [b], the drawn condition rows (indices into the gathered
# batch); ids1 / am1 [3 b, S], the triplet's token ids and masks [own | own | hard-negative text]; fetch(cond, neg_c) -> the drawn rows'
# condition tokens.
_ItmDraw = collections.namedtuple("_ItmDraw", "neg_c ids1 am1 fetch")


def _itm_draw(batch, st, sim_c2t, sim_t2c, row0, text, text_all):
    """The ITM hard negatives of sub-task `st` (vast.py:421-437): injected, or drawn per row and direction from the softmax of the similarities.
    row0: this rank's first row in the gathered batch; text / text_all: (ids, mask) of this rank / gathered."""
    inj, world = batch.get("_injected", {}), batch.get("_world")
    (ids, am), (ids_all, mask_all) = text, text_all
    bs, dev = ids.shape[0], ids.device
    if st in inj:
        neg_c, neg_t = inj[st]["neg_cond_idx"].to(dev), inj[st]["neg_text_idx"].to(dev)
    else:
        # one kernel per direction: softmax + 1e-4, own-rank diagonal zeroed, inverse-CDF draw per row (mico_itm_sample) - the
        # reference loops over rows with a .item() host sync each (vast.py:428-440); `_itm_uniform` injects the random numbers
        un = inj.get("_itm_uniform", {}).get(st)
        u_c, u_t = (un[0].to(dev), un[1].to(dev)) if un is not None else (torch.rand(bs, device=dev), torch.rand(bs, device=dev))
        neg_c = ops.itm_sample(sim_t2c.detach(), row0, u_c.float())
        neg_t = ops.itm_sample(sim_c2t.detach(), row0, u_t.float())
    return _ItmDraw(neg_c, torch.cat((ids, ids, ids_all[neg_t]), dim=0), torch.cat((am, am, mask_all[neg_t]), dim=0),
                    world[f"cond_{st[1:]}_fetch"] if world else D.fetch_rows)


def _itm_loss(self, ids1, am1, *, kv=None, cond3=None):
    """The ITM pass over the triplet [own | hard negative | own] and its loss (vast.py:438-457), against the shared K/V memory kv = (kv_own,
    kv_neg) of BertModel.project_cross_kv or the triplet's condition tokens cond3 [3 b, E, D]."""
    bs = ids1.shape[0] // 3
    out = self.multimodal_encoder.bert(input_ids=ids1, attention_mask=am1, encoder_hidden_states=cond3, cross_kv=kv).last_hidden_state
    logits = self.itm_head(out[:, 0])
    gt = torch.zeros(bs * 3, dtype=torch.long, device=ids1.device)
    gt[:bs] = 1
    return self.itm_ratio * Fn.cross_entropy(logits, gt)


def _itm_direct(self, enc, key, cond, draw):
    """The direct step's use of a draw, at once: the ITM loss of condition set `key` with the condition tokens `cond`."""
    cond_neg = draw.fetch(cond, draw.neg_c)
    if not _share_cross_kv(self):
        return _itm_loss(self, draw.ids1, draw.am1, cond3=torch.cat((cond, cond_neg, cond), dim=0))
    # the triplet [own | hard negative | own] holds the batch's own condition tokens twice and the captioning pass reads
    # them again: their K/V projections are computed once per step (functional.CrossKVFn) and kept for _forward_cap
    kv = enc.setdefault("_cross_kv", {})[key] = self.multimodal_encoder.bert.project_cross_kv(cond, cond_neg)
    return _itm_loss(self, draw.ids1, draw.am1, kv=kv)


def _forward_ret(self, batch, enc, subtasks, itm=True, deferred=None):
    """ITC + ITM of vast.py:395-457: per sub-task the contrastive loss, the hard-negative draw and the triplet pass, in this order.
    itm=False: the contrastive objective alone (step-A of SURVEY.md section 8d, BASELINE configs[1]) - nothing is drawn, no ITM pass is run
    and no "loss_itm" is returned (task prefix "itc%...", an addition of this repo).
    deferred (dict, the staged step): the draws are made, in the same order, and left in deferred[subtask] for _forward_staged, which runs
    the passes; only "loss_itc" is returned."""
    world = batch.get("_world")
    ids, am = _tokens(self, batch)
    rank = world["rank"] if world else D.rank()
    bs = ids.shape[0]
    feat_t = enc["feat_t"]
    feats = {st: _feat_cond(self, enc, st[1:]) for st in subtasks}
    if world:
        feat_t_all, ids_all, mask_all = world["feat_t_all"], world["ids_all"], world["mask_all"]
        feats_all = {st: world[f"feat_{st[1:]}_all"] for st in subtasks}
    else:   # ONE packed collective for every small per-step tensor (reference: 3 + len(subtasks) all_gathers)
        packed = D.packed_all_gather([feat_t, ids, am] + [feats[st] for st in subtasks])
        feat_t_all, ids_all, mask_all = packed[0], packed[1], packed[2]
        feats_all = dict(zip(subtasks, packed[3:]))
    targets = torch.arange(rank * bs, rank * bs + bs, device=ids.device)
    loss_itc, loss_itm = [], []
    for st in subtasks:
        fc, fc_all = feats[st], feats_all[st]
        sim_c2t = Fn.matmul_nt(fc, feat_t_all) / self.contra_temp                       # vast.py:405-408
        sim_t2c = Fn.matmul_nt(feat_t, fc_all) / self.contra_temp
        loss_itc.append((Fn.cross_entropy(sim_c2t, targets, 0.1) + Fn.cross_entropy(sim_t2c, targets, 0.1)) / 2)
        if itm:
            cond = _condition_feats(self, enc, st[1:]) if deferred is None else None       # (in front of the draw: the direct step's launch order)
            draw = _itm_draw(batch, st, sim_c2t, sim_t2c, rank * bs, (ids, am), (ids_all, mask_all))
            if deferred is None:
                loss_itm.append(_itm_direct(self, enc, st[1:], cond, draw))
            else:
                deferred[st] = draw
    out = {"loss_itc": sum(loss_itc) / len(loss_itc)}
    if loss_itm:
        out["loss_itm"] = sum(loss_itm) / len(loss_itm)
    return out


def _cap_inputs(self, batch):
    """masked token ids, labels (TokenMasker at 0.6 or the injected draw) and the causal 3-D mask of the captioning pass (vast.py:489-499)."""
    inj = batch.get("_injected", {})
    ids, am = _tokens(self, batch)
    if "cap" in inj:
        masked_ids, labels = inj["cap"]["masked_ids"].to(ids.device), inj["cap"]["labels"].to(ids.device)
    else:
        masked_ids, labels = self.text_masker(ids, 0.6)
    S = am.shape[1]
    m3 = torch.tril(am.unsqueeze(1).expand(-1, S, -1)).contiguous()                       # vast.py:497-499
    return masked_ids, labels, m3


def _twin_kv_own(self, offered, key):
    """kv_own of the retrieval twin whose K/V memory a captioning sub-task of condition set `key` reads, None if it projects its own tokens.
    offered: {condition set: (kv_own, kv_neg)} - in the direct step every memory once its triplet pass has projected it (enc["_cross_kv"]: a
    captioning family in front of its retrieval twin finds nothing), in the staged step the memory of a condition set's only triplet."""
    kv = offered.get(key) if _share_cross_kv(self) else None
    return None if kv is None else kv[0]


def _cap_loss(self, cap_in, *, kv_own=None, cond=None):
    """The captioning pass and its loss (vast.py:500-512) over cap_in = _cap_inputs(...), against _twin_kv_own's memory or, without one, cond."""
    masked_ids, labels, m3 = cap_in
    return self.multimodal_encoder(input_ids=masked_ids, attention_mask=m3, labels=labels, cross_kv=None if kv_own is None else (kv_own, None),
                                   encoder_hidden_states=cond if kv_own is None else None).loss


def _forward_cap(self, batch, enc, subtasks):
    cap_in = _cap_inputs(self, batch)
    losses = []
    for st in subtasks:
        kv_own = _twin_kv_own(self, enc.get("_cross_kv", {}), st[1:])
        losses.append(_cap_loss(self, cap_in, kv_own=kv_own, cond=_condition_feats(self, enc, st[1:]) if kv_own is None else None))
    return {"loss_cap": sum(losses) / len(losses)}


def qa_attention_mask(question_mask, answer_mask):
    """The part-causal 3-D mask of the QA pass (vast.py:594-599) from the key-padding masks [b, Lq], [b, La] -> {0, 1} [b, Lq + La, Lq + La]:
    padded keys are hidden from every row, question rows see the question only (bidirectional), answer rows see the question and the answer
    positions up to their own (prefix LM)."""
    Lq = question_mask.shape[1]
    keys = torch.cat((question_mask, answer_mask), dim=1)
    S = keys.shape[1]
    see = torch.ones(S, S, dtype=keys.dtype, device=keys.device).tril_()     # key j <= query i ...
    see[:, :Lq] = 1                                                          # ... or key j in the question
    return (keys.unsqueeze(1) * see.unsqueeze(0)).contiguous()


def _qa_questions(self, batch):
    """question ids / mask [nq, Lq] and the number of questions per sample (None: one each), from question_ids / question_mask
    (+ num_questions) or raw_questions - a list of str, or for evaluation a list of lists of str (vast.py:562-573)."""
    if "question_ids" in batch:
        nq = batch.get("num_questions")
        return batch["question_ids"], batch["question_mask"], None if nq is None else [int(n) for n in nq]
    raw, nq = batch["raw_questions"], None
    if any(isinstance(q, (list, tuple)) for q in raw):
        nq = [len(q) for q in raw]
        raw = [q for qs in raw for q in qs]
    return _tokenize(self, list(raw), self.max_caption_len) + (nq,)


def _qa_inputs(self, batch, q_ids, q_mask):
    """[question | masked answer] ids, the answer part's labels [b, La] (TokenMasker at 0.99 or the injected draw) and the part-causal mask of the
    QA pass (vast.py:580-599).  The labels of the question part are all -100 and are not materialised: only answer rows reach the LM head."""
    if "answer_ids" in batch:
        a_ids, a_mask = batch["answer_ids"], batch["answer_mask"]
    else:
        a_ids, a_mask = _tokenize(self, list(batch["raw_answers"]), self.max_answer_len)
    if a_ids.shape[0] != q_ids.shape[0]:
        raise ValueError(f"forward_qa: {q_ids.shape[0]} questions for {a_ids.shape[0]} answers (training takes one question per sample)")
    inj = batch.get("_injected", {})
    if "qa" in inj:
        masked_ids, labels = inj["qa"]["masked_ids"].to(q_ids.device), inj["qa"]["labels"].to(q_ids.device)
    else:
        masked_ids, labels = self.text_masker(a_ids, 0.99)
    return torch.cat((q_ids, masked_ids), dim=1), labels, qa_attention_mask(q_mask, a_mask)


def _cls_prompt(self, rows, device, prefix=None):
    """The decoding prompt [prefix | [CLS]] and its 3-D mask (vast.py:618-623); prefix: (ids [rows, L], key-padding mask [rows, L]) or None."""
    me = self.multimodal_encoder
    cls = torch.full((rows, 1), me.tokenizer.bos_token_id, dtype=torch.long, device=device)
    if prefix is None:
        return cls, cls.new_ones(rows, 1, 1)
    ids, m = prefix
    return torch.cat((ids, cls), dim=1), me.update_attention_mask(m.unsqueeze(1).expand(-1, ids.shape[1], -1).contiguous())


def _generate_text(self, cond, max_new_tokens, prefix=None, **search):
    """Decoded continuations of the prompt [prefix | [CLS]] under the condition tokens `cond`: BertForMaskedLM.generate (eos [SEP]; `search`:
    its beam-search or sampling arguments; config decode_use_cache: the cached decode), then the tokenizer over the new ids.
    Beam search also reads the config keys decode_device_search (the search itself on the device), decode_repetition_penalty,
    decode_no_repeat_ngram_size and decode_min_new_tokens (generate()'s logits processors); all default off.
    Sampling (do_sample in `search`) with the config key decode_device_sampling goes through BertForMaskedLM.sample instead (the step on the
    device), which also reads decode_top_p, decode_temperature and the three processor keys above; with the key off nothing changes.
    prefix: (ids [rows, L], mask [rows, L]) or None - one prompt row [CLS] per condition set."""
    me = self.multimodal_encoder
    tk = me.tokenizer
    prompt, mask = _cls_prompt(self, cond.shape[0] if prefix is None else prefix[0].shape[0], cond.device, prefix)
    if not search.get("do_sample", False):
        cfg = self.config
        for key, arg, off in (("decode_device_search", "device_search", False), ("decode_repetition_penalty", "repetition_penalty", 1.0),
                              ("decode_no_repeat_ngram_size", "no_repeat_ngram_size", 0), ("decode_min_new_tokens", "min_new_tokens", 0)):
            if cfg.get(key, off) != off:
                search.setdefault(arg, cfg.get(key))
    common = dict(input_ids=prompt, attention_mask=mask, encoder_hidden_states=cond, max_new_tokens=max_new_tokens,
                  eos_token_id=tk.sep_token_id, pad_token_id=tk.pad_token_id, use_cache=bool(self.config.get("decode_use_cache", False)))
    if search.get("do_sample", False) and self.config.get("decode_device_sampling", False):
        cfg = self.config
        warp = {arg: cfg.get(key) for key, arg in (("decode_top_p", "top_p"), ("decode_temperature", "temperature"),
                                                   ("decode_repetition_penalty", "repetition_penalty"),
                                                   ("decode_no_repeat_ngram_size", "no_repeat_ngram_size"),
                                                   ("decode_min_new_tokens", "min_new_tokens")) if cfg.get(key, None) is not None}
        out = me.sample(**common, **warp, **{k: v for k, v in search.items() if k != "do_sample"})
    else:
        out = me.generate(**common, **search)
    return tk.batch_decode(out[:, prompt.shape[1]:], skip_special_tokens=True)


def forward_qa(self, batch, task, compute_loss=True):
    """Visual question answering, task strings "qa%tv", "qa%tva%tv", ... (vast.py:557-650).
    compute_loss=True: {"loss_qa"} - per sub-task one pass over [question | answer masked at 0.99] under qa_attention_mask with the sub-task's
    condition tokens, the masked-token loss over the ANSWER rows (the question's labels are all -100: its rows contribute neither to the value
    nor to a gradient, so they skip the 768 x 30522 head); the mean over sub-tasks.  Like a captioning sub-task without a retrieval twin the
    pass projects its own cross-attention K/V.  No staged (backward_scale) form.
    compute_loss=False: {"generated_answers_<st>": list[str]}, flat in question order - beam search (beam_size, max_answer_len new tokens,
    eos [SEP], length penalty 1) from the prompt [question | [CLS]].  A sample may carry any number of questions (raw_questions as a list of
    lists, or num_questions); config decode_use_cache: the cached decode, each sample's condition tokens projected once and shared by its
    questions' rows (BertForMaskedLM.generate(rows_per_condition=...)), otherwise one copy of them per question as the reference makes."""
    (_, subtasks), = _parse_task(task, "forward_qa")
    batch = dict(batch) if not isinstance(batch, dict) else batch
    enc = encode_batch(self, batch)
    q_ids, q_mask, num_questions = _qa_questions(self, batch)
    me = self.multimodal_encoder
    Lq = q_ids.shape[1]
    if compute_loss:
        if num_questions is not None and any(n != 1 for n in num_questions):
            raise ValueError("forward_qa: several questions per sample are an evaluation input (compute_loss=False)")
        input_ids, labels, m3 = _qa_inputs(self, batch, q_ids, q_mask)
        losses = []
        for st in subtasks:
            cond = _condition_feats(self, enc, st[1:])
            seq = me.bert(input_ids=input_ids, attention_mask=m3, encoder_hidden_states=cond).last_hidden_state
            losses.append(Fn.LMHeadLossFn.apply(seq[:, Lq:], labels, *me._head_params()))
        return {"loss_qa": sum(losses) / len(losses)}
    out = {}
    for st in subtasks:
        cond = _condition_feats(self, enc, st[1:])
        rows = [1] * cond.shape[0] if num_questions is None else num_questions
        if q_ids.shape[0] == 0:
            out[f"generated_answers_{st}"] = []
            continue
        out[f"generated_answers_{st}"] = _generate_text(self, cond, self.max_answer_len, prefix=(q_ids, q_mask), num_beams=self.beam_size,
                                                        length_penalty=1.0, rows_per_condition=rows)
    return out


def forward_scst(self, batch, task, reward_fn, num_samples=1, sample_noise=None):
    """Self-critical sequence training of the captioner (the reference's --scst_finetuning; model/bert.py:1230-2102), task strings "cap%tv",
    "cap%tva%tv", ...  Per sub-task and sample: one greedy caption (the baseline) and num_samples sampled ones from the full softmax
    (BertForMaskedLM.scst_rollout: max_caption_len new tokens from the prompt [CLS], eos [SEP]; config decode_use_cache picks the cached
    decode), decoded to strings, then
        reward_fn(captions: list[str], sample_index: list[int], batch) -> one float per caption
    is called once for the greedy captions (sample_index = 0 .. b - 1) and once for the sampled ones (row b * num_samples + i belongs to sample
    b: sample_index = [0] * num_samples + [1] * num_samples + ...).  The project ships no reward (no CIDEr): reward_fn is the caller's, it sees
    the batch for its references (e.g. batch["raw_captions"]), and only reward differences matter.  With the advantage
    a[row] = r_sample[row] - r_greedy[sample of row] and logprobs = sequence_logprobs(sampled ids) (one differentiable two-stream pass over the
    SAMPLED rows only, its own cross-attention K/V projected from the expanded condition tokens),
        loss_scst = - sum_rows,t a[row] * logprobs[row, t] / #(sampled tokens up to and including each row's eos),
    averaged over sub-tasks; gradients reach BERT, the LM head and, through the condition tokens, the towers, as for loss_cap.
    sample_noise: fp32 [b * num_samples, max_caption_len] uniform numbers in [0, 1) for the draws (or {sub-task: such a tensor}); None: torch's
    generator.  Returns {"loss_scst", "reward_sample", "reward_greedy" (means, fp32 scalars), "sampled_captions_<st>", "greedy_captions_<st>"}.
    No staged (backward_scale) form."""
    (_, subtasks), = _parse_task(task, "forward_scst")
    if not callable(reward_fn):
        raise TypeError("forward_scst: reward_fn(captions, sample_index, batch) -> sequence of float is required (the project ships no reward)")
    K = int(num_samples)
    if K < 1:
        raise ValueError(f"forward_scst: num_samples = {num_samples}")
    batch = dict(batch) if not isinstance(batch, dict) else batch
    me = self.multimodal_encoder
    tk = me.tokenizer
    T = int(self.max_caption_len)
    use_cache = bool(self.config.get("decode_use_cache", False))
    # (the towers and the condition packing only: the caption text is the reward's business, no text pass is needed here)
    enc = encode_batch(self, {k: v for k, v in batch.items() if k not in ("raw_captions", "input_ids", "attention_mask", "caption_tokens")})
    out, losses, r_s_all, r_g_all, owner = {}, [], [], [], None
    for st in subtasks:
        cond = _condition_feats(self, enc, st[1:])
        b = cond.shape[0]
        owner = owner or [i // K for i in range(b * K)]      # the sample of each sampled row: one list for all sub-tasks
        noise = sample_noise.get(st) if isinstance(sample_noise, dict) else sample_noise
        prompt, mask = _cls_prompt(self, b, cond.device)
        roll = dict(max_new_tokens=T, eos_token_id=tk.sep_token_id, pad_token_id=tk.pad_token_id, use_cache=use_cache)
        g_ids, _ = me.scst_rollout(prompt, mask, cond.detach(), do_sample=False, **roll)
        s_ids, _ = me.scst_rollout(prompt, mask, cond.detach(), do_sample=True, sample_noise=noise, num_return_sequences=K, **roll)
        logp = me.sequence_logprobs(s_ids, mask.repeat_interleave(K, dim=0), cond.repeat_interleave(K, dim=0), prompt_len=1,
                                    eos_token_id=tk.sep_token_id, pad_token_id=tk.pad_token_id)
        caps_g = tk.batch_decode(g_ids[:, 1:], skip_special_tokens=True)
        caps_s = tk.batch_decode(s_ids[:, 1:], skip_special_tokens=True)
        r_g = torch.as_tensor(list(reward_fn(caps_g, list(range(b)), batch)), dtype=torch.float32, device=logp.device)
        r_s = torch.as_tensor(list(reward_fn(caps_s, owner, batch)), dtype=torch.float32, device=logp.device)
        if r_g.shape != (b,) or r_s.shape != (b * K,):
            raise ValueError(f"forward_scst: reward_fn returned {r_g.numel()} / {r_s.numel()} rewards for {b} / {b * K} captions")
        adv = r_s - r_g.repeat_interleave(K)
        n_valid = first_eos_valid(s_ids[:, 1:], tk.sep_token_id).sum().clamp_min(1).to(torch.float32)
        losses.append(-(adv[:, None] * logp).sum() / n_valid.to(logp.device))
        r_s_all.append(r_s.mean())
        r_g_all.append(r_g.mean())
        out[f"sampled_captions_{st}"], out[f"greedy_captions_{st}"] = caps_s, caps_g
    out["loss_scst"] = sum(losses) / len(losses)
    out["reward_sample"], out["reward_greedy"] = sum(r_s_all) / len(r_s_all), sum(r_g_all) / len(r_g_all)
    return out


class _StagedLoss(torch.autograd.Function):
    """The hand-over of a staged step (forward(backward_scale=...)): `value` is a loss that has ALREADY been differentiated through BERT inside
    forward, `grads[i]` = d(scale * sum of the staged losses) / d(tensors[i]) for the tower-side tensors the BERT passes read (the per-modality
    condition tokens).  The caller's backward of scale * (sum of the returned losses) arrives here with grad_output = scale and hands those
    gradients to the towers' graph (multiplied by grad_output / scale on the device - 1 when the caller keeps its side of the contract)."""

    @staticmethod
    def forward(ctx, value, scale, n, *tg):
        ctx.scale, ctx.n, ctx.grads = scale, n, tg[n:]
        return value.detach().clone()

    @staticmethod
    def backward(ctx, go):
        if ctx.grads is None:
            raise RuntimeError("_StagedLoss: a second backward through a staged step - its BERT side was differentiated inside the forward and the "
                               "condition-token gradients were handed over (scaled in place) by the first one; run the forward again")
        f = (go / ctx.scale).to(torch.float32)
        grads, ctx.grads = ctx.grads, None
        return (None, None, None) + tuple(g.mul_(f) for g in grads) + (None,) * ctx.n


def _acc(total, term):
    return term if total is None else total + term


def _forward_staged(self, batch, families, enc, scale):
    """forward(compute_loss=True) with the BERT passes differentiated ONE CONDITION SET AT A TIME inside the forward (round 6).
    The direct form builds every ITM / captioning graph, their cross-attention K/V memories and, in the backward, their gradients on top of the
    towers' complete activation stash (profiles/r05_mem_trace.txt: the step's peak is the second triplet's BertFn.backward).  Here the towers'
    condition tokens are cut out of the graph (detached leaves, one per modality), and for each condition set (e.g. "va": the tva triplet + the
    captioning pass that shares its K/V memory) the losses are built AND differentiated at once with the factor the caller will apply (`scale`:
    GradScaler's loss scale, 1.0 without one) - BERT-side parameter gradients go to .grad right away, the token gradients accumulate on the
    leaves, and the set's graph, K/V memory and gradient buffers are gone before the next set is built.  The returned losses carry one
    _StagedLoss node that hands the accumulated token gradients to the towers when the caller differentiates the sum.  Same loss values and
    gradients as the direct form (its _itm_loss and _cap_loss on the same numbers; only the order in which autograd sums the token gradients
    differs); random draws (hard negatives, token masks) happen in the direct form's order, BERT's per-pass dropout seeds are drawn in pass
    order, which differs.  families: _parse_task's list, none twice.  Contract: the caller calls backward() ONCE on scale * (unit-weight sum
    of the returned losses), after zero_grad - parameter gradients of the BERT side are already in .grad when forward returns."""
    ret_sub, cap_sub, out, deferred = [], [], {}, {}
    for kind, subtasks in families:
        if kind == "ret":
            out.update(_forward_ret(self, batch, enc, subtasks, deferred=deferred))
            ret_sub += subtasks
        elif kind == "itc":
            out.update(_forward_ret(self, batch, enc, subtasks, itm=False))
        else:
            cap_sub += subtasks
    cap_in = _cap_inputs(self, batch) if cap_sub else None
    leaves = {}
    sums = {"loss_itm": None, "loss_cap": None}
    for key in dict.fromkeys(st[1:] for st in ret_sub + cap_sub):      # the condition sets, in order of first mention
        for m in key:
            if m not in leaves:
                leaves[m] = enc["condition_feats_" + m].detach().requires_grad_(True)
        cond = torch.cat([leaves[m] for m in key], dim=1) if len(key) > 1 else leaves[key]
        total, offered = None, {}
        itm_sts = [st for st in ret_sub if st[1:] == key]
        for st in itm_sts:
            d = deferred[st]
            kv = self.multimodal_encoder.bert.project_cross_kv(cond, d.fetch(cond, d.neg_c))
            if len(itm_sts) == 1:      # (two triplets of one condition set: neither memory is the captioning pass's)
                offered[key] = kv
            l = _itm_loss(self, d.ids1, d.am1, kv=kv) / len(ret_sub)
            sums["loss_itm"], total = _acc(sums["loss_itm"], l.detach()), _acc(total, l)
            del kv
        for st in cap_sub:
            if st[1:] == key:
                l = _cap_loss(self, cap_in, kv_own=_twin_kv_own(self, offered, key), cond=cond) / len(cap_sub)
                sums["loss_cap"], total = _acc(sums["loss_cap"], l.detach()), _acc(total, l)
        del offered
        runtime.mem_trace("staged set " + key + ": graph built")
        with D.staged_backward():
            torch.autograd.backward(total * scale)
        del total, l, cond
        runtime.mem_trace("staged set " + key)
    first = True
    for k, v in sums.items():
        if v is None:
            continue
        if first and leaves:      # ONE node carries every condition-token gradient
            ms = list(leaves)
            v = _StagedLoss.apply(v, float(scale), len(ms), *[enc["condition_feats_" + m] for m in ms], *[leaves[m].grad for m in ms])
            first = False
        out[k] = v
    return out


def _eval_ret(self, batch, enc, subtasks):
    """evaluation dict of vast.py:466-483: the text feature and tokens, per sub-task the contrastive feature and the condition tokens"""
    ids, am = _tokens(self, batch)
    out = dict(feat_t=enc["feat_t"], input_ids=ids, attention_mask=am)
    for st in subtasks:
        out[f"feat_cond_{st}"] = _feat_cond(self, enc, st[1:])
        out[f"condition_feats_{st}"] = _condition_feats(self, enc, st[1:])
    return out


def _eval_cap(self, batch, enc, subtasks):
    """evaluation dict of vast.py:513-547: beam-search captions per sub-task, or with config captioner_mode generate_nums sampled captions per
    sample (top-k 10, vast.py:519-536), rows sample-major; with config decode_use_cache they share the sample's cross-attention K/V, with
    decode_device_sampling the sampling step runs on the device (_generate_text)."""
    out = {}
    for st in subtasks:
        cond = _condition_feats(self, enc, st[1:])
        if self.config.get("captioner_mode", False):
            gn = int(self.config.generate_nums)
            cached = bool(self.config.get("decode_use_cache", False))
            if not cached:      # a copy of the condition tokens per caption
                cond = cond.unsqueeze(1).expand(-1, gn, -1, -1).reshape(-1, *cond.shape[1:]).contiguous()
            search = dict(do_sample=True, top_k=10, sample_noise=(batch.get("_injected") or {}).get("sample_noise"),
                          num_return_sequences=gn if cached else 1)
        else:
            search = dict(num_beams=self.beam_size, length_penalty=0.6)
        out[f"generated_captions_{st}"] = _generate_text(self, cond, self.max_caption_len, **search)
    return out


def forward(self, batch, task, compute_loss=True, backward_scale=None):
    """Returns {"loss_itc", "loss_itm", "loss_cap"} for task strings like "ret%tva%tv_cap%tva" (vast.py:317-348); compute_loss=False: _eval_ret /
    _eval_cap.  The question-answering family ("qa%...") is not routed here - it raises NotImplementedError; call forward_qa.
    backward_scale (float; None = the direct form): staged differentiation, see _forward_staged - the factor the caller multiplies the summed
    losses with before its single backward() (1.0, or GradScaler.get_scale())."""
    families = _parse_task(task, "forward")
    kinds = [kind for kind, _ in families]
    if "itc" in kinds and not compute_loss:
        raise ValueError("itc%... is a training objective")
    batch = dict(batch) if not isinstance(batch, dict) else batch
    runtime.mem_trace("step start")
    # (a task string that names a branch twice keeps the direct form, whose later branch overwrites the earlier one's losses - vast.py:317-348)
    staged = backward_scale is not None and compute_loss and torch.is_grad_enabled() and _share_cross_kv(self) and len(set(kinds)) == len(kinds)
    runtime.step_staged = staged      # (functional.tower_plan: a staged step needs less memory next to the towers' saved activations)
    try:
        enc = encode_batch(self, batch)
    finally:
        runtime.step_staged = False   # (the plan is made inside the tower's forward: a tower pass outside MiCo.forward is priced as a direct step)
    runtime.mem_trace("after encode_batch")
    if staged:
        return _forward_staged(self, batch, families, enc, float(backward_scale))
    out = {}
    for kind, subtasks in families:
        if kind == "itc":      # contrastive objective only (no ITM passes): step-A of SURVEY.md section 8d
            out.update(_forward_ret(self, batch, enc, subtasks, itm=False))
        elif not compute_loss:
            out.update((_eval_ret if kind == "ret" else _eval_cap)(self, batch, enc, subtasks))
        elif kind == "ret":
            out.update(_forward_ret(self, batch, enc, subtasks))
            runtime.mem_trace("after forward_ret")
        else:
            out.update(_forward_cap(self, batch, enc, subtasks))
            runtime.mem_trace("after forward_cap")
    return out
