"""Plain-torch fp32 restatement of the question-answering pass (data/model/vast.py:557-650) on top of the CPU oracle's BERT
(oracle.mico_oracle.bert_mlm / encode_batch).  A helper for tests/test_qa_cpu.py and tests/test_qa_gpu.py, not a test."""
import torch

from oracle import mico_oracle as O


def qa_mask(question_mask, answer_mask):
    """vast.py:594-599 entry by entry: mask[b, i, j] = key j of sample b is no pad AND (j is a question position, or i and j are answer
    positions with j <= i)."""
    b, Lq = question_mask.shape
    La = answer_mask.shape[1]
    keys = torch.cat((question_mask, answer_mask), dim=1)
    out = torch.zeros(b, Lq + La, Lq + La, dtype=keys.dtype)
    for i in range(Lq + La):
        for j in range(Lq + La):
            if j < Lq or (i >= Lq and j <= i):
                out[:, i, j] = keys[:, j]
    return out


def qa_inputs(question_ids, question_mask, masked_answer_ids, answer_labels, answer_mask):
    """[question | masked answer] ids, labels (-100 over the question) and the 3-D mask of the pass (vast.py:588-599)."""
    ids = torch.cat((question_ids, masked_answer_ids), dim=1)
    labels = torch.cat((torch.full_like(question_ids, -100), answer_labels), dim=1)
    return ids, labels, qa_mask(question_mask, answer_mask)


def qa_loss(sd, arch, batch, fx, subtasks):
    """loss_qa of forward_qa(compute_loss=True): one bert_mlm pass per sub-task over every row, the mean.  batch: the towers' inputs;
    fx: question_ids / question_mask / masked_ids / labels / answer_mask.  Returns (loss, {sub-task: loss})."""
    enc = O.encode_batch(sd, arch, batch)
    ids, labels, m3 = qa_inputs(fx["question_ids"], fx["question_mask"], fx["masked_ids"], fx["labels"], fx["answer_mask"])
    each = {st: O.bert_mlm(sd, ids, m3, O.condition_feats(enc, st[1:]), labels)["loss"] for st in subtasks}
    return sum(each.values()) / len(each), each


def qa_prompt(question_ids, question_mask, bos=101):
    """The answer decode's prompt [question | [CLS]] and its mask: the question's key padding as [nq, Lq, Lq], grown once (vast.py:618-623)."""
    nq, Lq = question_ids.shape
    ids = torch.cat((question_ids, torch.full((nq, 1), bos, dtype=torch.long)), dim=1)
    return ids, O.grow_mask(question_mask[:, None, :].expand(nq, Lq, Lq).contiguous())


def beam_search_with_margins(step_logits, ids0, mask0, num_beams, max_new_tokens, eos=102, pad=0, length_penalty=1.0):
    """Beam search of BertForMaskedLM.generate (transformers 4.31 semantics, as oracle.mico_oracle.generate_beam restates them) from an
    arbitrary prompt ids0 [B, n] / mask0 [B, n, n], over step_logits(ids, mask) -> fp32 [B * num_beams, V], which also measures how decided
    each returned answer was.  Returns (ids [B, <= n + max_new_tokens], margin, top): `top` the largest |logit| seen, `margin` the smallest,
    over the prompt rows, of
      - at every step, the score of the returned hypothesis' prefix minus the score of the best candidate the selection left out (the prefix
        stays in the beam under any smaller perturbation of the scores);
      - where [SEP] is among the 2 num_beams + 1 best candidates of the row at a step (its rank decides whether a hypothesis is finished),
        every gap between them;
      - at the end, the returned hypothesis' score minus the runner-up's, as a sum of log-probabilities per generated token.
    Deliberately NOT covered: the order in which the other beams continue.  With the synthetic weights the next-token logits depend little
    on the prefix, so the candidates "x then y" and "y then x" score within rounding of each other at almost every step: no seed separates
    those, and they do not carry the answer."""
    B, n0 = ids0.shape
    nb = num_beams
    ids, mask = ids0.repeat_interleave(nb, dim=0), mask0.repeat_interleave(nb, dim=0)
    running = torch.zeros(B, nb)
    running[:, 1:] = -1e9
    running = running.reshape(-1)
    kept = [float("inf")] * (B * nb)          # per beam: how safely its prefix has stayed in the beam so far
    finished, worst, closed = [[] for _ in range(B)], [1e9] * B, [False] * B
    max_length = n0 + max_new_tokens
    margin, top = float("inf"), 0.0

    def push(b, hyp, logp, safe):
        score = logp / (hyp.shape[-1] ** length_penalty)
        if len(finished[b]) < nb or score > worst[b]:
            finished[b].append((score, hyp, safe))
            if len(finished[b]) > nb:
                ranked = sorted((h[0], i) for i, h in enumerate(finished[b]))
                del finished[b][ranked[0][1]]
                worst[b] = ranked[1][0]
            else:
                worst[b] = min(score, worst[b])

    while True:
        logits = step_logits(ids, mask).float().cpu()
        top = max(top, logits.abs().max().item())
        logp = torch.log_softmax(logits, dim=-1) + running[:, None]
        V = logp.shape[-1]
        cand_s, cand_i = torch.topk(logp.view(B, nb * V), 2 * nb + 1, dim=1)
        new_s, new_t, new_src = torch.zeros(B, nb), torch.zeros(B, nb, dtype=torch.long), torch.zeros(B, nb, dtype=torch.long)
        new_kept = list(kept)
        length_now = ids.shape[1] + 1
        for b in range(B):
            if closed[b]:
                new_t[b] = pad
                continue
            if bool((cand_i[b] % V == eos).any()):
                margin = min(margin, float((cand_s[b, :-1] - cand_s[b, 1:]).min()))
            used = []
            for rank in range(2 * nb):
                t = int(cand_i[b, rank]) % V
                src = b * nb + int(cand_i[b, rank]) // V
                used.append(rank)
                if t == eos:
                    if rank < nb:
                        push(b, ids[src].clone(), float(cand_s[b, rank]), kept[src])
                    continue
                k = sum(1 for r in used if int(cand_i[b, r]) % V != eos) - 1
                new_s[b, k], new_t[b, k], new_src[b, k] = cand_s[b, rank], t, src
                if k == nb - 1:
                    break
            left_out = float(cand_s[b, used[-1] + 1])
            k = 0
            for r in used:
                if int(cand_i[b, r]) % V != eos:
                    new_kept[b * nb + k] = min(kept[b * nb + int(cand_i[b, r]) // V], float(cand_s[b, r]) - left_out)
                    k += 1
            if len(finished[b]) >= nb and worst[b] >= float(cand_s[b].max()) / length_now ** length_penalty:
                closed[b] = True
        running, kept = new_s.reshape(-1), new_kept
        ids = torch.cat([ids[new_src.reshape(-1)], new_t.reshape(-1, 1)], dim=1)
        mask = O.grow_mask(mask)
        if all(closed) or ids.shape[1] >= max_length:
            break
    picks = []
    for b in range(B):
        if not closed[b]:
            for k in range(nb):
                push(b, ids[b * nb + k], float(running[b * nb + k]), kept[b * nb + k])
        ranked = sorted(finished[b], key=lambda h: h[0])
        margin = min(margin, ranked[-1][2])
        if len(ranked) > 1:
            # (scores are sums of step log-probabilities over the hypothesis' length, prompt included: the gap is put back per generated token)
            margin = min(margin, (ranked[-1][0] - ranked[-2][0]) * len(ranked[-1][1]) ** length_penalty / max(len(ranked[-1][1]) - n0, 1))
        picks.append(ranked[-1][1])
    width = min(max(len(h) for h in picks) + 1, max_length)
    out = torch.full((B, width), pad, dtype=torch.long)
    for b, h in enumerate(picks):
        out[b, :len(h)] = h
        if len(h) < width:
            out[b, len(h)] = eos
    return out, margin, top


def eval_case(seed, k=4, lo=1.5, hi=4.5):
    """The evaluation test's seeded case: six questions [6, 8] (question 1 with trailing pads) and a small 'answer vocabulary' - k token ids
    with LM-head bias boosts in [lo, hi) that lift them above the 30522 nearly flat logits of the synthetic weights, so that beam decisions
    stand further apart than 16-bit rounding while the ranking among the boosted tokens still depends on question and condition."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(1000, 30000, (6, 8), generator=g)
    q[:, 0] = 101
    qm = torch.ones(6, 8, dtype=torch.long)
    qm[1, 5:] = 0
    q[1, 4] = 102
    q[[0, 2, 3, 4, 5], 7] = 102
    toks = torch.randperm(29000, generator=g)[:k] + 1000
    boost = lo + (hi - lo) * torch.rand(k, generator=g)
    return q * qm, qm, toks, boost


SHARPEN = 4.0


def sharpen_keys(layers=12):
    """State-dict keys of the self-attention query / key projections of the multimodal BERT.  The evaluation test multiplies them by SHARPEN:
    with the synthetic weights as they are, self-attention is nearly uniform, the next-token logits then hardly depend on the ORDER of the
    prefix, and hypotheses that are permutations of each other ("x y" / "y x") tie within 16-bit rounding at every step whatever the seed.
    Peaked attention makes the order count, so that a seed without near-ties exists."""
    return [f"multimodal_encoder.bert.encoder.layer.{i}.attention.self.{n}.weight" for i in range(layers) for n in ("query", "key")]


CROSS_GAIN = 6.0


def cross_value_keys(layers=12):
    """State-dict keys of the cross-attention value projections.  The evaluation test multiplies them by CROSS_GAIN so that the condition
    tokens move the logits by more than the margins asked for: the samples then get different answers, and reading the wrong sample's
    K/V could not go unnoticed."""
    return [f"multimodal_encoder.bert.encoder.layer.{i}.crossattention.self.value.weight" for i in range(layers)]
