"""Host-side mirror of the reference's BERT-with-cross-attention text head (model/bert.py:81-1108): same module tree and
parameter names (`bert.embeddings.*`, `bert.encoder.layer.N.*`, `cls.predictions.*`), same call surface
(BertForMaskedLM(input_ids, attention_mask[2-D|3-D], encoder_hidden_states, labels) -> obj with .loss / .logits /
.sequence_output), arithmetic in mico_amd.functional.BertFn / LMHeadLossFn on libmico_hip.so.

BERT_CONFIG restates model/bert-base-uncased-crossattn/config.json (shape contract).
"""
import os

import torch
from torch import nn

from .. import functional as Fn, ops

BERT_CONFIG = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                   max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0,
                   hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, add_cross_attention=True, is_decoder=True)

TOKENIZER_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tokenizer")


class _Embeddings(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c["vocab_size"], c["hidden_size"], padding_idx=c["pad_token_id"])
        self.position_embeddings = nn.Embedding(c["max_position_embeddings"], c["hidden_size"])
        self.token_type_embeddings = nn.Embedding(c["type_vocab_size"], c["hidden_size"])
        self.LayerNorm = nn.LayerNorm(c["hidden_size"], eps=c["layer_norm_eps"])
        self.register_buffer("position_ids", torch.arange(c["max_position_embeddings"]).expand((1, -1)))


class _SelfAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        h = c["hidden_size"]
        self.query, self.key, self.value = nn.Linear(h, h), nn.Linear(h, h), nn.Linear(h, h)


class _SelfOutput(nn.Module):
    def __init__(self, c, in_features=None):
        super().__init__()
        self.dense = nn.Linear(in_features or c["hidden_size"], c["hidden_size"])
        self.LayerNorm = nn.LayerNorm(c["hidden_size"], eps=c["layer_norm_eps"])


class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.self = _SelfAttention(c)
        self.output = _SelfOutput(c)


class _Intermediate(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c["hidden_size"], c["intermediate_size"])


class _Layer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attention = _Attention(c)
        self.crossattention = _Attention(c)
        self.intermediate = _Intermediate(c)
        self.output = _SelfOutput(c, c["intermediate_size"])


class _Encoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(c) for _ in range(c["num_hidden_layers"])])


class _Out(dict):
    """attr-dict like the reference's easydict return value (bert.py:1093-1097)."""
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v


def extended_attention_mask(attention_mask):
    """bert.py:697-781: 2-D [b,S] key mask or 3-D [b,S,S] -> additive fp32 (1 - m) * -10000 (no automatic causal mask)."""
    if attention_mask.dim() not in (2, 3):
        raise ValueError(f"Wrong shape for attention_mask (shape {tuple(attention_mask.shape)})")
    return ((1.0 - attention_mask.to(torch.float32)) * -10000.0).contiguous()


def two_stream_inputs(input_ids, attention_mask, prompt_len, mask_token_id):
    """The inputs of the one-pass scoring of finished sequences under the [MASK]-append protocol (BertForMaskedLM.sequence_logprobs).
    input_ids [R, L] = a prompt of P = prompt_len positions and T = L - P generated ones; attention_mask: the prompt's {0, 1} mask
    [R, P, P], or that mask already grown to [R, L, L] (update_attention_mask, call it G).  Returns (ids [R, S2], mask [R, S2, S2],
    position ids [S2]) with S2 = (L - 1) + T:
      token stream  positions 0 .. L - 2 hold the real ids under G[:, :L-1, :L-1]; they see no column of the mask stream;
      mask stream   one [MASK] per generated position t = P .. L - 1, position id t: it sees the token columns j < t with G[t, j] = 1 and
                    itself - not token column t, no other [MASK].
    That is the row the [MASK] had when it was appended at step t, and since no position attends to a later one the token stream's rows are
    what they were at every step: the T mask-stream outputs are the T steps' outputs.  Pure torch; runs on CPU tensors as well."""
    R, L = input_ids.shape
    P = int(prompt_len)
    T = L - P
    if P < 1 or T < 1:
        raise ValueError(f"two_stream_inputs: a prompt of {P} and {T} generated positions in ids of length {L}")
    G = attention_mask
    if G.dim() != 3 or G.shape[0] != R or G.shape[1] != G.shape[2] or G.shape[1] not in (P, L):
        raise ValueError(f"two_stream_inputs: attention_mask {tuple(G.shape)} is neither the prompt's [{R}, {P}, {P}] nor the grown [{R}, {L}, {L}]")
    while G.shape[1] < L:
        G = BertForMaskedLM.update_attention_mask(G)
    dev = input_ids.device
    S2 = L - 1 + T
    ids = torch.cat((input_ids[:, :L - 1], torch.full((R, T), int(mask_token_id), dtype=input_ids.dtype, device=dev)), dim=1)
    mask = G.new_zeros(R, S2, S2)
    mask[:, :L - 1, :L - 1] = G[:, :L - 1, :L - 1]
    t = torch.arange(P, L, device=dev)
    earlier = (torch.arange(L - 1, device=dev)[None, :] < t[:, None]).to(G.dtype)           # [T, L - 1]: token column j < t
    mask[:, L - 1:, :L - 1] = G[:, P:, :L - 1] * earlier
    k = torch.arange(T, device=dev)
    mask[:, L - 1 + k, L - 1 + k] = 1
    return ids, mask, torch.cat((torch.arange(L - 1, device=dev), t))


def first_eos_valid(tokens, eos_token_id):
    """bool [R, T]: position t of row r is at or before the row's first eos (all True without an eos id) - the generated positions that
    count; everything after is padding."""
    if eos_token_id is None:
        return torch.ones_like(tokens, dtype=torch.bool)
    is_eos = (tokens == int(eos_token_id)).long()
    return (is_eos.cumsum(1) - is_eos) == 0


class BertModel(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.config = c
        self.embeddings = _Embeddings(c)
        self.encoder = _Encoder(c)
        self._spec = None
        self.dropout_seed_source = None   # callable -> int; None: one draw per pass from torch's host generator

    def _bert_spec(self):
        named = list(self.named_parameters())
        names = [n for n, _ in named]
        if self._spec is None or self._spec.names != names:
            self._spec = Fn.BertSpec(names, len(self.encoder.layer), self.config["num_attention_heads"],
                                     self.config["hidden_size"], self.config["intermediate_size"], self.config["layer_norm_eps"])
        return self._spec, [p for _, p in named]

    def project_cross_kv(self, cond_own, cond_neg=None):
        """Cross-attention K/V memory of condition tokens for all layers, to be shared by several passes of one training step
        (`cross_kv=` of forward): (kv_own, kv_neg) for the batch's own tokens [b, E, D] and, optionally, ITM hard negatives.
        Differentiable with respect to the tokens and the key / value projections (functional.CrossKVFn).
        Without grad (evaluation): no autograd node and no gradient session; cond_own may be 16-bit (the compute dtype) and kv_own is the
        interleaved [b E, L 2 D] memory that forward(cross_kv=kv_own, kv_index=...) reads by index."""
        spec, params = self._bert_spec()
        kvp = Fn.cross_kv_params(spec, params)
        if not torch.is_grad_enabled() and cond_neg is None:
            return Fn.cross_kv_memory(spec, cond_own, kvp), None
        session = Fn.DkvSession()
        kv_own, kv_neg = Fn.CrossKVFn.apply(spec, session, cond_own, cond_neg, *kvp)
        if kv_own.requires_grad:
            # the passes that read this memory find the session on the tensor (BertFn.forward) and keep ONE gradient buffer for the own set
            kv_own._mico_dkv = session
        return kv_own, kv_neg

    def forward(self, input_ids=None, attention_mask=None, encoder_hidden_states=None, kv_cache=None, cross_kv=None, kv_index=None,
                kv_sets=None, position_ids=None, **_):
        """position_ids (int64 [S], None = arange(S)): one position id per sequence position, shared by all batch entries.
        kv_index (int32 [b], inference only) with cross_kv = the interleaved K/V memory of project_cross_kv under no_grad, [sets E, L 2 D]
        (kv_sets = sets) or viewed [sets, E, L 2 D]: batch entry i attends to set kv_index[i], so b is independent of the number of sets
        (retrieval re-ranking: every candidate projected once, read by all its pairs).  The values must lie in [0, sets).
        kv_cache (dict, inference only): holds the cross-attention K/V projections of `encoder_hidden_states` across calls -
        the caller guarantees the condition tokens do not change between the calls that share the dict.
        cross_kv (training): (kv_own, kv_neg) from project_cross_kv instead of encoder_hidden_states; a batch of b entries attends
        to kv_own, a batch of 3 b entries is the ITM triplet [own | hard negative | own] and needs kv_neg as well."""
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        spec, params = self._bert_spec()
        drop = None
        ph, pa = self.config["hidden_dropout_prob"], self.config["attention_probs_dropout_prob"]
        if self.training and (ph > 0 or pa > 0):
            # nn.Dropout sites of bert.py:148,267,295,373: masks come from a counter hash of (seed, site, element), one seed per pass
            seed = self.dropout_seed_source() if self.dropout_seed_source is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)))
            drop = (float(ph), float(pa), int(seed))
        if kv_cache is not None:
            if torch.is_grad_enabled() and any(p.requires_grad for p in params):
                raise RuntimeError("kv_cache is an inference feature: call under torch.no_grad()")
            drop = None      # (an inference pass: no dropout)
        kv_own, kv_neg = (None, None)
        if cross_kv is not None:
            if encoder_hidden_states is not None or kv_cache is not None:
                raise ValueError("cross_kv replaces encoder_hidden_states / kv_cache")
            kv_own, kv_neg = cross_kv if isinstance(cross_kv, (tuple, list)) else (cross_kv, None)
            if kv_index is not None:
                if torch.is_grad_enabled():
                    raise RuntimeError("kv_index is an inference feature (the indexed K/V memory has no backward): call under torch.no_grad()")
                if kv_neg is not None:
                    raise ValueError("kv_index reads one K/V memory: cross_kv is a single tensor")
                if kv_own.dim() == 3:
                    kv_sets, kv_own = kv_own.shape[0], kv_own.reshape(-1, kv_own.shape[-1])
                if not kv_sets or kv_own.dim() != 2 or kv_own.shape[0] % int(kv_sets):
                    raise ValueError("kv_index needs cross_kv as [sets, E, L 2 D], or as [sets E, L 2 D] with kv_sets=sets")
                if kv_index.dtype != torch.int32 or kv_index.shape != (input_ids.shape[0],):
                    raise ValueError("kv_index is an int32 [batch] tensor")
                drop, kv_index = None, kv_index.contiguous()
            if kv_neg is not None and input_ids.shape[0] % 3:
                raise ValueError("cross_kv with hard negatives expects the ITM triplet batch [own | negative | own]")
        elif kv_index is not None:
            raise ValueError("kv_index needs cross_kv")
        if position_ids is not None:
            if position_ids.dtype != torch.long or position_ids.shape != (input_ids.shape[1],):
                raise ValueError(f"position_ids is an int64 [{input_ids.shape[1]}] tensor, one id per sequence position")
            position_ids = position_ids.to(input_ids.device).contiguous()
        seq = Fn.BertFn.apply(spec, input_ids, extended_attention_mask(attention_mask), encoder_hidden_states, drop, kv_own, kv_neg,
                              kv_cache, kv_index, int(kv_sets or 0), position_ids, *params)
        return _Out(last_hidden_state=seq)


class _Transform(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c["hidden_size"], c["hidden_size"])
        self.LayerNorm = nn.LayerNorm(c["hidden_size"], eps=c["layer_norm_eps"])


class _Predictions(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.transform = _Transform(c)
        self.decoder = nn.Linear(c["hidden_size"], c["vocab_size"], bias=False)
        self.bias = nn.Parameter(torch.zeros(c["vocab_size"]))
        self.decoder.bias = self.bias   # bert.py:604


class _MLMHead(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.predictions = _Predictions(c)


class _LazyLogits:
    def __init__(self, fn):
        self._fn, self._v = fn, None

    def get(self):
        if self._v is None:
            self._v = self._fn()
        return self._v


class _MLMOut(_Out):
    """`.logits` is computed on first access: the reference always evaluates the 768x30522 LM head (bert.py:1085) even when
    only .sequence_output is consumed; results are identical, the wasted GEMM is not."""

    def __getattr__(self, k):
        if k == "logits":
            lazy = dict.get(self, "_lazy_logits")
            return lazy.get() if lazy is not None else None
        return dict.get(self, k)


class BertForMaskedLM(nn.Module):
    def __init__(self, config=None):
        super().__init__()
        c = dict(BERT_CONFIG)
        if config:
            c.update(config)
        self.config = c
        self.bert = BertModel(c)
        self.cls = _MLMHead(c)
        self._init_weights()
        # weight tying (transformers==4.31 post_init via get_output_embeddings, bert.py:1038-1041)
        self.cls.predictions.decoder.weight = self.bert.embeddings.word_embeddings.weight
        self.tokenizer = None

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                m.weight.data.normal_(mean=0.0, std=0.02)
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.Embedding):
                m.weight.data.normal_(mean=0.0, std=0.02)
                if m.padding_idx is not None:
                    m.weight.data[m.padding_idx].zero_()
            elif isinstance(m, nn.LayerNorm):
                m.bias.data.zero_()
                m.weight.data.fill_(1.0)

    def get_output_embeddings(self):
        return self.cls.predictions.decoder

    def _head_params(self):
        pr = self.cls.predictions
        return (pr.transform.dense.weight, pr.transform.dense.bias, pr.transform.LayerNorm.weight, pr.transform.LayerNorm.bias,
                pr.decoder.weight, pr.bias)

    def forward(self, input_ids=None, attention_mask=None, encoder_hidden_states=None, labels=None, cross_kv=None, **_):
        seq = self.bert(input_ids, attention_mask, encoder_hidden_states, cross_kv=cross_kv).last_hidden_state
        out = _MLMOut(loss=None, sequence_output=seq)
        hp = self._head_params()
        if labels is not None:
            out["loss"] = Fn.LMHeadLossFn.apply(seq, labels, *hp)
        dict.__setitem__(out, "_lazy_logits", _LazyLogits(lambda: Fn.LMLogitsFn.apply(seq.detach(), *[p.detach() for p in hp])))
        return out

    # ---- caption decoding (inference_demo.py:161-171; the [MASK]-append protocol of bert.py:1110-1143) -------------------------
    @staticmethod
    def update_attention_mask(attention_mask):
        """bert.py:1110-1117: grow a [b,n,n] mask to [b,n+1,n+1]; the new row copies the last row and sees itself."""
        b, n, _ = attention_mask.shape
        up = attention_mask.new_zeros(b, n + 1, n + 1)
        up[:, :n, :n] = attention_mask
        up[:, n, :n] = attention_mask[:, n - 1, :n]
        up[:, n, n] = 1
        return up

    def prepare_inputs_for_generation(self, input_ids, attention_mask=None, encoder_hidden_states=None, **_):
        """bert.py:1126-1143: append one [MASK] token whose output row predicts the next token."""
        dummy = torch.full((input_ids.shape[0], 1), self.tokenizer.mask_token_id, dtype=torch.long, device=input_ids.device)
        return {"input_ids": torch.cat([input_ids, dummy], dim=1), "attention_mask": self.update_attention_mask(attention_mask),
                "encoder_hidden_states": encoder_hidden_states}

    @torch.no_grad()
    def next_token_logits(self, input_ids, attention_mask, encoder_hidden_states, kv_cache=None):
        """One decode step of the reference protocol: logits [rows, vocab] of the appended [MASK] position.  Only that row
        goes through the 768x30522 LM head (the reference evaluates it for every position and slices, bert.py:1085); with a
        kv_cache dict the cross-attention K/V of the condition tokens are projected once per decode, not once per step."""
        inp = self.prepare_inputs_for_generation(input_ids, attention_mask, encoder_hidden_states)
        seq = self.bert(inp["input_ids"], inp["attention_mask"], inp["encoder_hidden_states"], kv_cache=kv_cache).last_hidden_state
        last = seq[:, -1:, :].contiguous()
        return Fn.LMLogitsFn.apply(last, *[p.detach() for p in self._head_params()])[:, 0, :]

    def _decode_cache(self, input_ids, attention_mask, cond, rows_per_set, max_length):
        """functional.BertDecodeCache for a decode of input_ids / attention_mask ([rows, n], [rows, n, n]) that reaches max_length
        positions; cond [rows / rows_per_set, E, D] (one condition set per rows_per_set consecutive rows; rows_per_set a list: set s is
        read by rows_per_set[s] consecutive rows) or None."""
        mask = attention_mask
        while mask.shape[1] < max_length:
            mask = self.update_attention_mask(mask)
        spec, params = self.bert._bert_spec()
        return Fn.BertDecodeCache(spec, params, self._head_params(), cond, rows_per_set, mask, self.tokenizer.mask_token_id)

    def _model_step(self, input_ids, attention_mask, cond, rows_per_set, max_length, use_cache):
        """The model step of a decode, an object with next_token_logits(ids, parent=None): the cached one (_decode_cache), or the
        recomputing one over one copy of the condition tokens per row (arguments as _decode_cache's)."""
        if use_cache:
            return self._decode_cache(input_ids, attention_mask, cond, rows_per_set, max_length)
        if cond is not None and not isinstance(rows_per_set, int):     # (the row -> set index is built on the host: no device-side size query)
            own = torch.arange(len(rows_per_set)).repeat_interleave(torch.tensor(rows_per_set))
            cond = cond[own.to(cond.device)]
        elif cond is not None and rows_per_set != 1:
            cond = cond.repeat_interleave(rows_per_set, dim=0)
        return _RecomputingStep(self, attention_mask, cond)

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, encoder_hidden_states=None, max_new_tokens=20, num_beams=1,
                 eos_token_id=None, pad_token_id=None, length_penalty=1.0, do_sample=False, top_k=50, sample_noise=None,
                 use_cache=False, num_return_sequences=1, rows_per_condition=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_length=0, min_new_tokens=0, device_search=False, done_check_every=1, **unused):
        """Beam search with the semantics of transformers==4.31 GenerationMixin.generate / BeamSearchScorer as the reference
        calls it (inference_demo.py:164-171: num_beams 3, length_penalty 0.6, early_stopping False, no logits processors by default):
        2*num_beams candidates per step, finished hypotheses scored sum_logprob / len**length_penalty, the "cannot improve"
        stop heuristic, finalisation with the open beams, eos-terminated pad-filled output.  The search bookkeeping runs on
        the host over 2*num_beams candidates per sample; the model step and log-softmax / top-k run on the device.
        top_k = 0 (sampling): no top-k warper, as in transformers - one draw per row and step from the full softmax on the device
        (mico_vocab_sample; _rollout), `sample_noise`, num_return_sequences and use_cache as for top-k sampling.
        use_cache: incremental decoding (functional.BertDecodeCache) - one pass over the prompt, then 2 positions per row and step;
        the rows of one condition set (beams, sampled captions) share its cross-attention K/V.  Same ids as the recomputing path up to
        floating-point reduction order.  num_return_sequences (sampling only): n rows per condition set, sample-major.
        rows_per_condition (beam search only; None: one prompt row per condition set): a sequence of ints, one per set of
        encoder_hidden_states - set s is read by rows_per_condition[s] consecutive prompt rows (question answering: a sample's questions;
        zero allowed).  With the cache each set is projected once and read through the ragged decode attention; without it the condition
        tokens are expanded here, one copy per prompt row.
        Logits processors (beam search only, all off by default; apply_logits_processors): repetition_penalty, no_repeat_ngram_size,
        min_length (eos banned while a row is shorter, prompt included) / min_new_tokens (while fewer tokens have been generated).  They act
        on the log-probabilities over a row's whole ids, prompt included, as in transformers' beam_search.  num_beams = 1 runs the same beam
        program, so repetition_penalty follows beam_search's order there too (penalty on log-probabilities), not transformers' greedy_search
        (penalty on raw logits); the two -inf processors are the same either way.
        device_search (beam search only, num_beams <= 8): the search itself on the device - per step mico_beam_topk (log-softmax, processors,
        the 2 num_beams best per prompt row; equal scores by ascending beam * vocab + token, where torch.topk leaves the order open) and
        mico_beam_step (BeamSearchScorer's bookkeeping), mico_beam_finalize at the end; the host reads one counter of unfinished prompt rows
        every done_check_every steps and the lengths once.  Steps taken after every row has finished change nothing, so the ids do not
        depend on done_check_every.  Same ids as the host search wherever its decisions do not hang on an fp32 rounding of the log-softmax."""
        if unused:
            raise TypeError(f"generate(): unsupported arguments {sorted(unused)}")
        pen, ngram, min_len, min_new = float(repetition_penalty), int(no_repeat_ngram_size), int(min_length), int(min_new_tokens)
        if pen <= 0:
            raise ValueError(f"generate(): repetition_penalty = {repetition_penalty} (a positive number; 1: off)")
        if ngram < 0 or min_len < 0 or min_new < 0:
            raise ValueError(f"generate(): no_repeat_ngram_size {no_repeat_ngram_size}, min_length {min_length}, min_new_tokens {min_new_tokens}: "
                             "none may be negative")
        if int(done_check_every) < 1:
            raise ValueError(f"generate(): done_check_every = {done_check_every} (at least 1)")
        if device_search and int(num_beams) > ops.BEAM_NB_MAX:
            raise ValueError(f"generate(): device_search takes num_beams <= {ops.BEAM_NB_MAX} (got {num_beams})")
        processors = pen != 1.0 or ngram > 0 or min_len > 0 or min_new > 0
        if do_sample and (processors or device_search or int(done_check_every) != 1):
            raise ValueError("generate(): repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens, device_search and "
                             "done_check_every are provided for beam search only (do_sample=False)")
        rpc = None
        if rows_per_condition is not None:      # (checked before anything is launched)
            rpc = [int(r) for r in rows_per_condition]
            if do_sample:
                raise ValueError("generate(): rows_per_condition is provided for beam search only")
            if encoder_hidden_states is None or len(rpc) != encoder_hidden_states.shape[0]:
                raise ValueError(f"generate(): rows_per_condition has {len(rpc)} entries for "
                                 f"{0 if encoder_hidden_states is None else encoder_hidden_states.shape[0]} condition sets")
            if any(r < 0 for r in rpc):
                raise ValueError(f"generate(): rows_per_condition {rpc} holds a negative row count")
            if sum(rpc) != input_ids.shape[0]:
                raise ValueError(f"generate(): rows_per_condition {rpc} adds up to {sum(rpc)}, the prompt has {input_ids.shape[0]} rows")
        nrs = int(num_return_sequences)
        if nrs < 1 or (nrs != 1 and not do_sample):
            raise ValueError("generate(): num_return_sequences > 1 is provided for sampling (do_sample=True) only")
        if use_cache and self.training:
            raise RuntimeError("generate(use_cache=True) is inference-only (the cached decode has no BERT dropout): call .eval() first")
        if do_sample:
            if int(num_beams) != 1:
                raise TypeError("generate(): do_sample with num_beams > 1 (beam sampling) is not used by the reference and not provided")
            if nrs > 1:      # sample-major rows b * n + i (vast.py:519-536 expands the condition the same way)
                input_ids, attention_mask = input_ids.repeat_interleave(nrs, dim=0), attention_mask.repeat_interleave(nrs, dim=0)
            max_length = input_ids.shape[1] + int(max_new_tokens)
            if int(top_k) < 0:
                raise ValueError(f"generate(): top_k = {top_k} (0: no top-k warper, the full softmax)")
            dec = self._model_step(input_ids, attention_mask, encoder_hidden_states, nrs, max_length, use_cache)
            if int(top_k) == 0:
                return self._rollout(dec, input_ids, max_length, eos_token_id, pad_token_id, sample_noise, True)[0]
            return self._sample(dec, input_ids, max_length, int(top_k), eos_token_id, pad_token_id, sample_noise)
        dev = input_ids.device
        B, cur = input_ids.shape
        nb = int(num_beams)
        max_length = cur + int(max_new_tokens)
        ids = input_ids.repeat_interleave(nb, dim=0)
        dec = self._model_step(ids, attention_mask.repeat_interleave(nb, dim=0), encoder_hidden_states,
                               nb if rpc is None else [r * nb for r in rpc], max_length, use_cache)
        ban_eos = lambda n: eos_token_id is not None and (n < min_len or n - cur < min_new)      # n: the rows' length before the step
        if device_search:
            return self._device_beam_search(dec, ids, nb, max_length, eos_token_id, pad_token_id, length_penalty,
                                            (pen, ngram, ban_eos) if processors else None, int(done_check_every))
        beam_scores = torch.zeros(B, nb, dtype=torch.float32, device=dev)
        beam_scores[:, 1:] = -1e9
        beam_scores = beam_scores.view(-1)
        hyps = [_BeamHypotheses(nb, length_penalty) for _ in range(B)]
        done = [False] * B
        parent = None
        while True:
            logits = dec.next_token_logits(ids, parent).float()
            if processors:
                scores = apply_logits_processors(torch.log_softmax(logits, dim=-1), ids, eos_token_id, pen, ngram, ban_eos(ids.shape[1]))
                scores = scores + beam_scores[:, None]
            else:
                scores = torch.log_softmax(logits, dim=-1) + beam_scores[:, None]
            V = scores.shape[-1]
            top_s, top_i = torch.topk(scores.view(B, nb * V), 2 * nb, dim=1, largest=True, sorted=True)
            top_s, top_i = top_s.cpu(), top_i.cpu()
            src_beam, tok = top_i // V, top_i % V
            ids_cpu = ids.cpu()
            cur_len = ids.shape[1] + 1
            nxt_s = torch.zeros(B, nb)
            nxt_t = torch.zeros(B, nb, dtype=torch.long)
            nxt_b = torch.zeros(B, nb, dtype=torch.long)
            for b in range(B):
                if done[b]:
                    nxt_t[b] = pad_token_id
                    continue
                k = 0
                for rank in range(2 * nb):
                    row = b * nb + int(src_beam[b, rank])
                    if eos_token_id is not None and int(tok[b, rank]) == eos_token_id:
                        if rank >= nb:
                            continue
                        hyps[b].add(ids_cpu[row].clone(), float(top_s[b, rank]))
                    else:
                        nxt_s[b, k], nxt_t[b, k], nxt_b[b, k] = top_s[b, rank], tok[b, rank], row
                        k += 1
                    if k == nb:
                        break
                done[b] = done[b] or hyps[b].is_done(float(top_s[b].max()), cur_len)
            beam_scores = nxt_s.view(-1).to(dev)
            parent = nxt_b.view(-1)
            ids = torch.cat([ids[parent.to(dev)], nxt_t.view(-1, 1).to(dev)], dim=1)
            if all(done) or ids.shape[1] >= max_length:
                break
        ids_cpu, fin = ids.cpu(), beam_scores.cpu()
        best = []
        for b in range(B):
            if not done[b]:
                for k in range(nb):
                    hyps[b].add(ids_cpu[b * nb + k], float(fin[b * nb + k]))
            best.append(max(hyps[b].beams, key=lambda h: h[0])[1])
        lens = [int(h.shape[0]) for h in best]
        width = min(max(lens) + 1, max_length)
        out = torch.full((B, width), pad_token_id if pad_token_id is not None else 0, dtype=torch.long)
        for b, h in enumerate(best):
            out[b, :lens[b]] = h
            if lens[b] < width:
                out[b, lens[b]] = eos_token_id
        return out.to(dev)

    def _device_beam_search(self, dec, ids0, nb, max_length, eos_token_id, pad_token_id, length_penalty, processors, check_every):
        """generate()'s beam search with the search on the device: ids0 [sets nb, P] the prompt rows times nb; processors None or
        (repetition_penalty, no_repeat_ngram_size, ban_eos(length) -> bool).  The rows' ids live in the two halves of an int64
        [rows, max_length] double buffer (a step gathers the parents' prefixes from one half into the other); the model step sees the
        filled columns as a view and re-gathers its cache by the device-side parents."""
        dev = ids0.device
        rows, cur = ids0.shape
        sets = rows // nb
        pad = int(pad_token_id) if pad_token_id is not None else 0
        buf = [torch.full((rows, max_length), pad, dtype=torch.long, device=dev) for _ in range(2)]
        buf[0][:, :cur] = ids0
        beam_scores = torch.zeros(sets, nb, dtype=torch.float32, device=dev)
        beam_scores[:, 1:] = -1e9
        beam_scores = beam_scores.view(-1)
        state = ops.BeamState(sets, nb, max_length, length_penalty, dev)
        parent = torch.empty(rows, dtype=torch.long, device=dev)
        cand, side, steps = None, 0, 0
        while cur < max_length:
            ids = buf[side][:, :cur]
            logits = dec.next_token_logits(ids, parent if steps else None).float()
            proc = {}
            if processors is not None:
                proc = dict(ids=ids, repetition_penalty=processors[0], no_repeat_ngram_size=processors[1], ban_eos=processors[2](cur),
                            eos_token_id=eos_token_id)
            cand = ops.beam_topk(logits, beam_scores, nb, done=state.done, out=cand, **proc)
            ops.beam_step(state, cand, buf[side], buf[side ^ 1], cur, beam_scores, parent, eos_token_id=eos_token_id, pad_token_id=pad)
            side, cur, steps = side ^ 1, cur + 1, steps + 1
            if cur < max_length and steps % check_every == 0 and int(state.not_done.item()) == 0:      # the step's only host read
                break
        best, lens = ops.beam_finalize(state, buf[side], cur, beam_scores, eos_token_id=eos_token_id, pad_token_id=pad)
        width = min(int(lens.max()) + 1, max_length) if sets else cur
        return best[:, :width].contiguous()

    def _sample(self, dec, ids, max_length, top_k, eos_token_id, pad_token_id, noise):
        """Top-k sampling as the reference's captioner_mode asks transformers 4.31 for it (vast.py:526-536: do_sample=True, top_k=10,
        temperature 1): per step the top_k logits are kept (TopKLogitsWarper), softmax over them, ONE draw per row; rows that have
        produced eos emit pad from then on; stop when every row has finished or max_length is reached.  The draw is inverse-CDF over
        the kept candidates in descending-score order with one uniform number per (row, step): `noise` [rows, max_new_tokens] injects
        them (parity tests), otherwise they come from torch's generator - the same distribution as torch.multinomial, not the same
        stream.  Device: model step (dec, of _model_step) + top-k; host: k candidates per row."""
        dev = ids.device
        B = ids.shape[0]
        unfinished = torch.ones(B, dtype=torch.bool)
        step = 0
        while True:
            logits = dec.next_token_logits(ids).float()
            top_s, top_i = torch.topk(logits, min(top_k, logits.shape[-1]), dim=-1, largest=True, sorted=True)
            probs = torch.softmax(top_s, dim=-1).cpu().double()
            top_i = top_i.cpu()
            u = noise[:, step].double().cpu() if noise is not None else torch.rand(B, dtype=torch.float64)
            cdf = probs.cumsum(-1)
            pick = (cdf < (u * cdf[:, -1])[:, None]).sum(-1).clamp_max(probs.shape[-1] - 1)
            tok = top_i[torch.arange(B), pick]
            if eos_token_id is not None:
                tok = torch.where(unfinished, tok, torch.full_like(tok, pad_token_id if pad_token_id is not None else 0))
                unfinished = unfinished & (tok != eos_token_id)
            ids = torch.cat([ids, tok.view(-1, 1).to(dev)], dim=1)
            step += 1
            if not bool(unfinished.any()) or ids.shape[1] >= max_length:
                break
        return ids

    def _rollout(self, dec, ids, max_length, eos_token_id, pad_token_id, noise, do_sample):
        """Decode loop on the device over the model step `dec` (of _model_step): per step ONE draw per row from the full softmax
        (ops.vocab_sample; uniform numbers from `noise` [rows, max_new_tokens] or torch's device generator) or, do_sample=False, the argmax.
        Rows that have produced eos emit pad from then on; stops when every row has finished or max_length is reached (one flag read per
        step, as _sample).  Returns (ids [rows, <= max_length], log P(chosen token) per step fp32 [rows, steps], 0 on finished rows)."""
        dev = ids.device
        B = ids.shape[0]
        pad = int(pad_token_id) if pad_token_id is not None else 0
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        step, logps = 0, []
        while True:
            logits = dec.next_token_logits(ids).float()
            if do_sample:
                u = noise[:, step].to(dev, torch.float32) if noise is not None else torch.rand(B, device=dev)
                tok, lp = ops.vocab_sample(logits, u, unfinished=unfinished if eos_token_id is not None else None,
                                              eos_token_id=eos_token_id, pad_token_id=pad)
            else:
                tok = logits.argmax(-1)
                lp = logits.gather(1, tok[:, None])[:, 0] - torch.logsumexp(logits, dim=-1)
                if eos_token_id is not None:
                    tok = torch.where(unfinished, tok, torch.full_like(tok, pad))
                    lp = torch.where(unfinished, lp, torch.zeros_like(lp))
                    unfinished = unfinished & (tok != eos_token_id)
            ids = torch.cat([ids, tok.view(-1, 1)], dim=1)
            logps.append(lp)
            step += 1
            if ids.shape[1] >= max_length or not bool(unfinished.any()):
                break
        return ids, torch.stack(logps, dim=1)

    @torch.no_grad()
    def sample(self, input_ids=None, attention_mask=None, encoder_hidden_states=None, max_new_tokens=20, top_k=0, top_p=1.0, temperature=1.0,
               repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0, eos_token_id=None, pad_token_id=None,
               num_return_sequences=1, use_cache=False, sample_noise=None, device_search=True, done_check_every=1, return_logprobs=False):
        """Sampling decode with the semantics of transformers==4.31 sample(): per step the logits processors on the raw logits
        (apply_logits_processors: repetition_penalty, no_repeat_ngram_size, the eos ban of min_length / min_new_tokens), then the warpers
        (apply_logits_warpers: temperature, top_k - 0: off, at most ops.SAMPLE_TOPK_MAX -, top_p), then ONE draw per row by inverse CDF with
        one uniform number per (row, step) - `sample_noise` [rows, max_new_tokens], or torch's generator.  The walk of the draw is in
        descending score order with top_k >= 1 (the order of generate(do_sample=True, top_k >= 1), whose ids this returns when only top_k is
        set) and in column order with top_k = 0 (the order of generate(do_sample=True, top_k=0)).  Rows that have produced eos emit pad from
        then on.  num_return_sequences, use_cache and the row expansion as in generate()'s sampling branch.
        device_search: the ids live in one int64 [rows, max_length] buffer; a step is one model step plus one mico_warp_sample, which also
        appends the token and keeps the unfinished flags and their count on the device; the host reads that count every done_check_every
        steps.  Steps taken after every row has finished only write pad, so the ids do not depend on done_check_every.
        device_search=False: the same program in torch (the unfinished flags are read every step).
        Returns ids [rows, <= max_length], trimmed after the step at which the last row finished; with return_logprobs also the per-step
        log-probabilities of the drawn tokens under the warped distribution, fp32 [rows, steps], 0 on finished rows."""
        k, top_p, temp, pen = int(top_k), float(top_p), float(temperature), float(repetition_penalty)
        ngram, min_len, min_new, T = int(no_repeat_ngram_size), int(min_length), int(min_new_tokens), int(max_new_tokens)
        nrs, check_every = int(num_return_sequences), int(done_check_every)
        if not 0 <= k <= ops.SAMPLE_TOPK_MAX:
            raise ValueError(f"sample(): top_k = {top_k} (0: no top-k warper; at most {ops.SAMPLE_TOPK_MAX})")
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"sample(): top_p = {top_p} (in (0, 1]; 1: off)")
        if not 0.0 < temp < float("inf"):
            raise ValueError(f"sample(): temperature = {temperature} (a positive number)")
        if pen <= 0:
            raise ValueError(f"sample(): repetition_penalty = {repetition_penalty} (a positive number; 1: off)")
        if ngram < 0 or min_len < 0 or min_new < 0:
            raise ValueError(f"sample(): no_repeat_ngram_size {no_repeat_ngram_size}, min_length {min_length}, min_new_tokens {min_new_tokens}: "
                             "none may be negative")
        if T < 1 or nrs < 1:
            raise ValueError(f"sample(): max_new_tokens = {max_new_tokens}, num_return_sequences = {num_return_sequences} (at least 1 each)")
        if check_every < 1:
            raise ValueError(f"sample(): done_check_every = {done_check_every} (at least 1)")
        if sample_noise is not None and tuple(sample_noise.shape) != (input_ids.shape[0] * nrs, T):
            raise ValueError(f"sample(): sample_noise is [rows, max_new_tokens] = [{input_ids.shape[0] * nrs}, {T}] uniform numbers")
        if use_cache and self.training:
            raise RuntimeError("sample(use_cache=True) is inference-only (the cached decode has no BERT dropout): call .eval() first")
        if nrs > 1:
            input_ids, attention_mask = input_ids.repeat_interleave(nrs, dim=0), attention_mask.repeat_interleave(nrs, dim=0)
        P = input_ids.shape[1]
        max_length = P + T
        dec = self._model_step(input_ids, attention_mask, encoder_hidden_states, nrs, max_length, use_cache)
        pad = int(pad_token_id) if pad_token_id is not None else 0
        warp = dict(top_k=k, top_p=top_p, temperature=temp)
        proc = dict(repetition_penalty=pen, no_repeat_ngram_size=ngram)
        ban_eos = lambda n: eos_token_id is not None and (n < min_len or n - P < min_new)      # n: the rows' length before the step
        run = self._device_sample if device_search else self._host_sample
        ids, logps = run(dec, input_ids, max_length, warp, proc, ban_eos, eos_token_id, pad, sample_noise, check_every)
        return (ids, logps) if return_logprobs else ids

    def _device_sample(self, dec, ids0, max_length, warp, proc, ban_eos, eos_token_id, pad, noise, check_every):
        """sample()'s loop with the step on the device (ops.warp_sample); returns (ids, logps)."""
        dev = ids0.device
        rows, P = ids0.shape
        T = max_length - P
        buf = torch.full((rows, max_length), pad, dtype=torch.long, device=dev)
        buf[:, :P] = ids0
        u = noise.to(dev, torch.float32).t().contiguous() if noise is not None else torch.rand(T, rows, device=dev)
        logps = torch.zeros(T, rows, dtype=torch.float32, device=dev)
        out = [torch.empty(rows, dtype=dt, device=dev) for dt in (torch.int64, torch.float32, torch.int32, torch.float32)]
        unfinished = not_done = None
        if eos_token_id is not None:
            unfinished = torch.ones(rows, dtype=torch.uint8, device=dev)
            not_done = torch.full((1,), rows, dtype=torch.int32, device=dev)
        processors = proc["repetition_penalty"] != 1.0 or proc["no_repeat_ngram_size"] > 0 or any(ban_eos(n) for n in range(P, max_length))
        steps = 0
        while steps < T:
            cur = P + steps
            logits = dec.next_token_logits(buf[:, :cur]).float()
            in_kernel = logits.shape[-1] <= 65536 and cur <= 512      # the processors' (and with them the append's) limits
            if processors and not in_kernel:
                raise ValueError(f"sample(): the device-side logits processors take a vocabulary <= 65536 and rows <= 512 ids "
                                 f"(got {logits.shape[-1]}, {cur})")
            ids_arg = dict(ids=buf, cur_len=cur, append=True, ban_eos=ban_eos(cur), **proc) if in_kernel else {}
            out[1] = logps[steps]
            ops.warp_sample(logits, u[steps], eos_token_id=eos_token_id, pad_token_id=pad, unfinished=unfinished, not_done=not_done,
                            out=tuple(out), **warp, **ids_arg)
            if not in_kernel:
                buf[:, cur] = out[0]
            steps += 1
            if not_done is not None and steps < T and steps % check_every == 0 and int(not_done.item()) == 0:      # the step's only host read
                break
        width = T
        if eos_token_id is not None:      # the step at which the last row finished (one read)
            hit = buf[:, P:P + steps] == eos_token_id
            first = torch.where(hit.any(dim=1), hit.int().argmax(dim=1) + 1, torch.full((rows,), steps, device=dev))
            width = int(first.max()) if rows else steps
        return buf[:, :P + width].contiguous(), logps[:width].t().contiguous()

    def _host_sample(self, dec, ids, max_length, warp, proc, ban_eos, eos_token_id, pad, noise, check_every):
        """sample()'s loop in torch: apply_logits_processors, apply_logits_warpers, the draw by a float64 CDF (in descending score order over
        the top_k candidates as _sample walks it, in column order with top_k = 0); returns (ids, logps)."""
        dev = ids.device
        B = ids.shape[0]
        k = warp["top_k"]
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        rows = torch.arange(B, device=dev)
        step, logps = 0, []
        while True:
            scores = apply_logits_processors(dec.next_token_logits(ids).float(), ids, eos_token_id, ban_eos=ban_eos(ids.shape[1]), **proc)
            warped, kept = apply_logits_warpers(scores, **warp)
            u = noise[:, step].to(dev).double() if noise is not None else torch.rand(B, dtype=torch.float64, device=dev)
            if k > 0:
                top_s, top_i = torch.sort(warped, dim=-1, descending=True, stable=True)
                top_s, top_i = top_s[:, :k], top_i[:, :k]
                cdf = torch.softmax(top_s, dim=-1).double().cumsum(-1)
                pick = (cdf < (u * cdf[:, -1])[:, None]).sum(-1).minimum(kept.sum(-1) - 1).clamp_min(0)
                tok = top_i[rows, pick]
            else:
                w = torch.softmax(warped.double(), dim=-1)
                cdf = w.cumsum(-1)
                last = (torch.arange(w.shape[1], device=dev) * (w > 0)).amax(-1)      # the last column with a weight
                tok = (cdf <= (u * cdf[:, -1])[:, None]).sum(-1).minimum(last)
            lp = warped[rows, tok] - torch.logsumexp(warped, dim=-1)
            empty = ~kept.any(-1)      # no finite score: token 0, log-prob -inf
            tok = torch.where(empty, torch.zeros_like(tok), tok)
            lp = torch.where(empty, torch.full_like(lp, float("-inf")), lp)
            if eos_token_id is not None:
                tok = torch.where(unfinished, tok, torch.full_like(tok, pad))
                lp = torch.where(unfinished, lp, torch.zeros_like(lp))
                unfinished = unfinished & (tok != eos_token_id)
            ids = torch.cat([ids, tok.view(-1, 1)], dim=1)
            logps.append(lp)
            step += 1
            if ids.shape[1] >= max_length or not bool(unfinished.any()):
                break
        return ids, torch.stack(logps, dim=1)

    @torch.no_grad()
    def scst_rollout(self, input_ids, attention_mask, encoder_hidden_states, max_new_tokens, eos_token_id, pad_token_id, do_sample=True,
                     sample_noise=None, num_return_sequences=1, use_cache=True):
        """The no-grad roll-out of generate_scst: (ids [R n, P + T], the roll-out's own log P(chosen token) fp32 [R n, T]) for R prompt
        rows, n = num_return_sequences rows per condition set (sample-major, sampling only) and T = max_new_tokens; both are padded
        (pad_token_id / 0) after a row's eos up to the full width.  The model runs without dropout, whatever self.training says."""
        nrs = int(num_return_sequences)
        if nrs < 1 or (nrs != 1 and not do_sample):
            raise ValueError("scst_rollout(): num_return_sequences > 1 is provided for sampling (do_sample=True) only")
        T = int(max_new_tokens)
        if T < 1:
            raise ValueError(f"scst_rollout(): max_new_tokens = {max_new_tokens}")
        if sample_noise is not None and (not do_sample or tuple(sample_noise.shape) != (input_ids.shape[0] * nrs, T)):
            raise ValueError(f"scst_rollout(): sample_noise is [rows, max_new_tokens] = [{input_ids.shape[0] * nrs}, {T}] uniform numbers "
                             "of a sampled roll-out")
        if nrs > 1:
            input_ids, attention_mask = input_ids.repeat_interleave(nrs, dim=0), attention_mask.repeat_interleave(nrs, dim=0)
        max_length = input_ids.shape[1] + T
        dec = self._model_step(input_ids, attention_mask, encoder_hidden_states, nrs, max_length, use_cache)
        ids, lp = self._rollout(dec, input_ids, max_length, eos_token_id, pad_token_id, sample_noise, do_sample)
        short = max_length - ids.shape[1]
        if short:      # every row finished early
            ids = torch.cat([ids, ids.new_full((ids.shape[0], short), int(pad_token_id) if pad_token_id is not None else 0)], dim=1)
            lp = torch.cat([lp, lp.new_zeros(lp.shape[0], short)], dim=1)
        return ids, lp

    def sequence_logprobs(self, input_ids, attention_mask, encoder_hidden_states=None, prompt_len=None, eos_token_id=None,
                          pad_token_id=None):
        """log P(token) of every generated position of finished sequences, fp32 [R, T], in ONE differentiable pass (two_stream_inputs:
        about 2 T rows per sequence instead of the reference's T passes over the growing prefix, bert.py:1230-2102).
        input_ids [R, P + T] with P = prompt_len; attention_mask: the prompt's 3-D mask [R, P, P] (or the grown [R, P + T, P + T]);
        encoder_hidden_states [R, E, D] or None.  Entry [r, t] = log softmax(logits of step t)[input_ids[r, P + t]]; positions after a
        row's first eos_token_id are exactly 0, value and gradient (they hold pad_token_id, which is not looked at).  Differentiable with
        respect to the BERT and LM-head parameters and encoder_hidden_states; BERT's dropout applies when self.training.  Only the T
        mask-stream rows go through the 768 x 30522 head (functional.LMHeadLogProbFn)."""
        if prompt_len is None:
            raise ValueError("sequence_logprobs(): prompt_len is required")
        P = int(prompt_len)
        L = input_ids.shape[1]
        ids2, mask2, pos = two_stream_inputs(input_ids, attention_mask, P, self.tokenizer.mask_token_id)
        if L > self.config["max_position_embeddings"]:
            raise ValueError(f"sequence_logprobs(): {L} positions exceed the position table")
        targets = input_ids[:, P:]
        targets = torch.where(first_eos_valid(targets, eos_token_id), targets, torch.full_like(targets, -100))
        seq = self.bert(ids2, mask2, encoder_hidden_states, position_ids=pos).last_hidden_state
        return Fn.LMHeadLogProbFn.apply(seq[:, L - 1:], targets, *self._head_params())

    def generate_scst(self, input_ids, attention_mask, encoder_hidden_states, max_new_tokens, eos_token_id, pad_token_id, do_sample=True,
                      sample_noise=None, num_return_sequences=1, use_cache=True, return_rollout_logprobs=False):
        """Self-critical sequence training's sampler (the reference's sample_scst, bert.py:1230-1502): (ids [R n, P + T], logprobs fp32
        [R n, T]) - ids from a no-grad roll-out (scst_rollout: one draw per step from the full softmax, or greedy with do_sample=False),
        logprobs = sequence_logprobs(ids) with a gradient, over condition tokens expanded to one copy per row.
        Two differences from the reference: the roll-out runs without dropout (with the cache it is the inference decode) while the
        scoring pass applies BERT's dropout when self.training; positions after a row's eos carry 0 (the reference leaves the log-prob of
        a token that is not in ids there, bert.py:1454-1461, and every caller masks it).
        return_rollout_logprobs: also the roll-out's own per-step log-probs [R n, T] (no gradient; tests tie the two paths with it)."""
        nrs = int(num_return_sequences)
        ids, step_lp = self.scst_rollout(input_ids, attention_mask, None if encoder_hidden_states is None else encoder_hidden_states.detach(),
                                         max_new_tokens, eos_token_id, pad_token_id, do_sample=do_sample, sample_noise=sample_noise,
                                         num_return_sequences=nrs, use_cache=use_cache)
        cond = encoder_hidden_states
        if nrs > 1:
            attention_mask = attention_mask.repeat_interleave(nrs, dim=0)
            cond = cond.repeat_interleave(nrs, dim=0) if cond is not None else None
        logprobs = self.sequence_logprobs(ids, attention_mask, cond, prompt_len=input_ids.shape[1], eos_token_id=eos_token_id,
                                          pad_token_id=pad_token_id)
        return (ids, logprobs, step_lp) if return_rollout_logprobs else (ids, logprobs)


def apply_logits_processors(scores, ids, eos_token_id, repetition_penalty=1.0, no_repeat_ngram_size=0, ban_eos=False):
    """transformers' RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and the eos ban of MinLength / MinNewTokensLength, in that
    order, as one pure-torch function on any device: scores [rows, V] (beam search: log-probabilities) and the rows' whole ids [rows, cur]
    -> processed scores (a new tensor).  A seen token's score s becomes s * p where s < 0, else s / p; with n = no_repeat_ngram_size > 0
    token t is -inf where ids[i .. i + n - 2] equals the last n - 1 ids and ids[i + n - 1] == t (n = 1: every seen token; nothing while
    cur < n); ban_eos: eos_token_id is -inf.  An id outside [0, V) names no score and is ignored (mico_beam_topk does the same)."""
    rows, V = scores.shape
    cur = ids.shape[1]

    def marked(tok, keep):      # bool [rows, V]: the tokens tok[keep]; the rest go to a spare column
        m = torch.zeros(rows, V + 1, dtype=torch.bool, device=scores.device)
        return m.scatter_(1, torch.where(keep & (tok >= 0) & (tok < V), tok, torch.full_like(tok, V)), True)[:, :V]

    if repetition_penalty != 1.0 and cur > 0:
        penalised = torch.where(scores < 0, scores * repetition_penalty, scores / repetition_penalty)
        scores = torch.where(marked(ids, torch.ones_like(ids, dtype=torch.bool)), penalised, scores)
    n = int(no_repeat_ngram_size)
    if n > 0 and cur >= n:
        windows = ids.unfold(1, n, 1)                                   # [rows, cur - n + 1, n]
        match = (windows[..., :-1] == ids[:, cur + 1 - n:].unsqueeze(1)).all(dim=-1)
        scores = scores.masked_fill(marked(windows[..., -1], match), float("-inf"))
    if ban_eos and eos_token_id is not None and 0 <= int(eos_token_id) < V:
        scores = scores.clone()
        scores[:, int(eos_token_id)] = float("-inf")
    return scores


def apply_logits_warpers(scores, top_k=0, top_p=1.0, temperature=1.0):
    """transformers' TemperatureLogitsWarper, TopKLogitsWarper and TopPLogitsWarper (min_tokens_to_keep 1), in that order, as one pure-torch
    function on any device: scores [rows, V] fp32 or fp64 (processed logits) -> (warped scores, -inf outside the kept set; kept mask, bool
    [rows, V]).  s = scores / temperature; top_k > 0 keeps the min(top_k, V) best of a stable descending sort, so equal scores go by
    ascending column (TopKLogitsWarper keeps every tie with the k-th score); top_p < 1 keeps, of the softmax over what is left, the candidate
    of descending rank r iff the probability mass of the ranks ahead of it is < top_p, rank 0 always (ties in that same order; the masses
    are summed in float64; top_p = 1: no cut).  A score of -inf is never kept.  mico_warp_sample does the same on the device."""
    s = scores if temperature == 1.0 else scores / torch.tensor(float(temperature), dtype=scores.dtype, device=scores.device)
    V = s.shape[-1]
    ranked, order = torch.sort(s, dim=-1, descending=True, stable=True)
    keep = ranked > float("-inf")
    if int(top_k) > 0:
        keep = keep & (torch.arange(V, device=s.device) < int(top_k))
    if float(top_p) < 1.0:
        probs = torch.softmax(ranked.double().masked_fill(~keep, float("-inf")), dim=-1)      # (float64 whatever the scores are)
        before = torch.cat([torch.zeros_like(probs[:, :1]), probs.cumsum(-1)[:, :-1]], dim=-1)      # mass of the ranks ahead
        head = torch.arange(V, device=s.device) == 0
        keep = keep & ((before < float(top_p)) | head)
    kept = torch.zeros_like(keep).scatter_(1, order, keep)
    return s.masked_fill(~kept, float("-inf")), kept


class _RecomputingStep:
    """The recomputing model step behind functional.BertDecodeCache's interface: every call runs all positions of ids plus the appended
    [MASK] (BertForMaskedLM.next_token_logits).  Owns the 3-D mask, grown by one position per generated token."""

    def __init__(self, model, attention_mask, enc):
        self.model, self.mask = model, attention_mask
        self.enc = enc.contiguous() if enc is not None else None
        # a row attends to the same condition tokens at every step and rows are only ever reordered within their condition set (beams), so
        # the per-layer cross-attention K/V of `enc` are step-invariant: projected at the first step, reused afterwards
        self.kv_cache = {} if enc is not None else None

    def next_token_logits(self, ids, parent=None):
        """parent: not needed - nothing here is kept per row (beams are reordered within their prompt row, whose mask they share)."""
        if self.mask.shape[1] < ids.shape[1]:
            self.mask = self.model.update_attention_mask(self.mask)
        return self.model.next_token_logits(ids, self.mask, self.enc, self.kv_cache)


class _BeamHypotheses:
    """n-best list of finished hypotheses of one sample (transformers==4.31 BeamHypotheses, early_stopping=False)."""

    def __init__(self, num_beams, length_penalty):
        self.num_beams, self.length_penalty = num_beams, length_penalty
        self.beams, self.worst_score = [], 1e9

    def add(self, hyp, sum_logprobs):
        score = sum_logprobs / (hyp.shape[-1] ** self.length_penalty)
        if len(self.beams) < self.num_beams or score > self.worst_score:
            self.beams.append((score, hyp))
            if len(self.beams) > self.num_beams:
                order = sorted((s, i) for i, (s, _) in enumerate(self.beams))
                del self.beams[order[0][1]]
                self.worst_score = order[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self.beams) < self.num_beams:
            return False
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty


def build_tokenizer():
    """BertTokenizer over the bert-base-uncased WordPiece vocabulary, with the special ids the reference sets
    (mico.py:109-113): bos=[CLS] 101, eos=[SEP] 102, pad=[PAD] 0, mask=[MASK] 103."""
    from transformers import BertTokenizer
    tok = BertTokenizer.from_pretrained(TOKENIZER_DIR)   # vocab.txt + tokenizer_config.json (mico.py:109)
    tok.bos_token_id = tok.convert_tokens_to_ids(["[CLS]"])[0]
    tok.eos_token_id = tok.convert_tokens_to_ids(["[SEP]"])[0]
    tok.pad_token_id = tok.convert_tokens_to_ids(["[PAD]"])[0]
    tok.mask_token_id = tok.convert_tokens_to_ids(["[MASK]"])[0]
    return tok
