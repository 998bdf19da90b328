"""Retrieval evaluation: ITC top-k, ITM re-ranking of the shortlist, R@1/5/10.

The consumer of the evaluation dictionary `MiCo.forward(batch, "ret%...", compute_loss=False)` returns (vast.py:466-483): the reference
scores a (text, candidate) pair with compute_slice_scores (vast.py:373-380) and re-ranks the itm_rerank_num best candidates of the
contrastive similarity (data/utils/args.py:259); the `evaluation` package that drives the two is not part of the reference.

Scheme.  The shortlists of both directions (text -> candidate, candidate -> text) are cut by ops.topk_rows; plan_pairs takes the union of
their (text, candidate) pairs, so a pair both directions ask for is scored once, and sorts it candidate-major.  The candidates are walked in
chunks that fit a K/V budget: a chunk's condition tokens (kept in 16 bits) are projected to the cross-attention K/V memory of all BERT
layers ONCE (BertModel.project_cross_kv), its pairs run through BERT in sub-batches that read that memory by index
(BertModel.forward(kv_index=...), mico_attn_params.kv_index), and the chunk is freed.  A per-pair evaluation projects a candidate's tokens
once per pair instead - k times for a shortlist of k.

Planning and metrics are plain torch index arithmetic and run on the CPU as well.  Single process: sharding the pair list over ranks is
not provided (every rank would evaluate everything).
"""
import collections

import torch
import torch.nn.functional as F

from . import ops, runtime
from . import functional as Fn

PairPlan = collections.namedtuple("PairPlan", "text cand inv_t2c inv_c2t")
PairPlan.__doc__ = """text, cand: int64 [P] - the distinct (text, candidate) pairs, sorted by candidate, then text.
inv_t2c: int64 [Nq, k] (or None) - pair number of (i, top_t2c[i, r]);  inv_c2t: int64 [Nc, k] (or None) - pair number of (top_c2t[j, r], j):
per_pair_score[inv_*] is the [., k] score table of that direction."""

KV_BUDGET_FRACTION = 0.25     # default K/V budget of a candidate chunk: this share of the free device memory, read once per process
_FREE_BYTES = None


def plan_pairs(top_t2c=None, top_c2t=None, n_text=None, n_cand=None):
    """Union of the pairs {(i, top_t2c[i, r])} and {(top_c2t[j, r], j)} (either table may be None), candidate-major, with the maps back
    into the two tables.  n_text / n_cand default to the tables' row counts (needed when only the other direction is given)."""
    if top_t2c is None and top_c2t is None:
        raise ValueError("plan_pairs needs the shortlist of at least one direction")
    n_text = n_text if n_text is not None else (top_t2c.shape[0] if top_t2c is not None else int(top_c2t.max()) + 1)
    n_cand = n_cand if n_cand is not None else (top_c2t.shape[0] if top_c2t is not None else int(top_t2c.max()) + 1)
    codes, shapes = [], []
    if top_t2c is not None:
        t = top_t2c.long()
        rows = torch.arange(t.shape[0], device=t.device).unsqueeze(1).expand_as(t)
        codes.append((t * n_text + rows).reshape(-1))         # code = candidate * n_text + text: sorting the codes is candidate-major
        shapes.append(("t2c", t.shape))
    if top_c2t is not None:
        t = top_c2t.long()
        rows = torch.arange(t.shape[0], device=t.device).unsqueeze(1).expand_as(t)
        codes.append((rows * n_text + t).reshape(-1))
        shapes.append(("c2t", t.shape))
    uniq, inverse = torch.unique(torch.cat(codes), sorted=True, return_inverse=True)
    inv, off = {"t2c": None, "c2t": None}, 0
    for name, shp in shapes:
        n = shp[0] * shp[1]
        inv[name] = inverse[off:off + n].view(shp)
        off += n
    cand = torch.div(uniq, n_text, rounding_mode="floor")
    if uniq.numel() and (int(cand.max()) >= n_cand or int(uniq.min()) < 0):
        raise ValueError("shortlist indices out of range")
    return PairPlan(uniq - cand * n_text, cand, inv["t2c"], inv["c2t"])


def plan_chunks(cand, max_cands):
    """Cuts the candidate-major pair list into chunks of at most max_cands distinct candidates; a candidate's pairs are never split.
    Returns a list of (cands int64 [m], p0, p1, kv_index int32 [p1 - p0]): the chunk's candidates in ascending order, its pair range and,
    per pair, the position of its candidate within `cands` (what the indexed attention reads)."""
    if max_cands < 1:
        raise ValueError("a chunk holds at least one candidate")
    if cand.numel() == 0:
        return []
    ucand, counts = torch.unique_consecutive(cand, return_counts=True)
    ends = torch.cumsum(counts, 0)
    rank = torch.repeat_interleave(torch.arange(ucand.numel(), device=cand.device), counts)     # per pair: number of its candidate in ucand
    out = []
    for c0 in range(0, ucand.numel(), max_cands):
        c1 = min(c0 + max_cands, ucand.numel())
        p0 = int(ends[c0 - 1]) if c0 else 0
        p1 = int(ends[c1 - 1])
        out.append((ucand[c0:c1], p0, p1, (rank[p0:p1] - c0).to(torch.int32)))
    return out


def kv_bytes_per_candidate(E, n_layers, hidden=768, elem_bytes=2):
    """Bytes of one candidate's cross-attention K/V memory over all layers: E tokens x L x (K | V)."""
    return E * n_layers * 2 * hidden * elem_bytes


def default_kv_budget(device):
    """KV_BUDGET_FRACTION of the device memory that was free at the first call (read once: the evaluation's own buffers must not shrink it)."""
    global _FREE_BYTES
    if _FREE_BYTES is None:
        _FREE_BYTES = torch.cuda.mem_get_info(device)[0]
    return int(_FREE_BYTES * KV_BUDGET_FRACTION)


def trimmed_length(attention_mask, multiple=16):
    """Text length that keeps every attended position of every row: the last attended position + 1, rounded up to `multiple`, at most S."""
    S = attention_mask.shape[1]
    if attention_mask.numel() == 0:
        return S
    pos = torch.arange(1, S + 1, device=attention_mask.device)
    longest = int(((attention_mask != 0) * pos).max())
    return min(S, max(multiple, -(-longest // multiple) * multiple))


@torch.no_grad()
def score_pairs(model, input_ids, attention_mask, condition_feats, plan, kv_budget_bytes=None, pair_batch=512, trim_text=True):
    """ITM score softmax(itm_head(BERT(text, candidate)[:, 0]))[:, 1] of every pair of `plan` (fp32 [P], on the model's device).
    condition_feats [Nc, E, D]: any device, fp32 or the compute dtype (stored 16-bit, they are projected as they are).  kv_budget_bytes:
    K/V memory of one candidate chunk (None: default_kv_budget).  pair_batch: pairs per BERT pass.  trim_text: cut each sub-batch's token
    rows to trimmed_length - the removed key columns are the ones the -10000 mask already zeroes (exp underflows to 0) and only the CLS row
    is read, so nothing a score depends on changes; False keeps the padded length."""
    bert = model.multimodal_encoder.bert
    dev = input_ids.device
    dt = runtime.compute_dtype()
    Nc, E, D = condition_feats.shape
    L = len(bert.encoder.layer)
    budget = default_kv_budget(dev) if kv_budget_bytes is None else int(kv_budget_bytes)
    max_cands = max(1, budget // kv_bytes_per_candidate(E, L, D, 2))
    scores = torch.empty(plan.text.numel(), dtype=torch.float32, device=dev)
    text_dev = plan.text.to(dev)
    am_host = attention_mask.cpu() if trim_text else None
    text_host = plan.text.cpu()
    stats = dict(chunks=0, bert_passes=0, kv_projections=0, pairs=int(plan.text.numel()), max_cands=int(max_cands))
    for cands, p0, p1, kv_index in plan_chunks(plan.cand, max_cands):
        cond = condition_feats[cands.to(condition_feats.device)].to(device=dev, dtype=dt)
        kv, _ = bert.project_cross_kv(cond)
        del cond
        stats["chunks"] += 1
        stats["kv_projections"] += int(cands.numel())
        kv_index = kv_index.to(dev)
        for q0 in range(p0, p1, pair_batch):
            q1 = min(q0 + pair_batch, p1)
            S = trimmed_length(am_host[text_host[q0:q1]]) if trim_text else input_ids.shape[1]
            rows = text_dev[q0:q1]
            out = bert(input_ids=input_ids[rows, :S], attention_mask=attention_mask[rows, :S], cross_kv=kv,
                       kv_index=kv_index[q0 - p0:q1 - p0], kv_sets=int(cands.numel())).last_hidden_state
            scores[q0:q1] = F.softmax(model.itm_head(out[:, 0]), dim=1)[:, 1]
            stats["bert_passes"] += 1
        del kv
    score_pairs.last_stats = stats
    return scores


def compose_order(topk_idx, itm_scores, full_order):
    """Final ranking per row: the k shortlisted entries by ITM score descending (equal scores keep their ITC order), then everything
    else in ITC order.  topk_idx [rows, k] must be full_order[:, :k]; full_order [rows, cols] is the ITC ranking."""
    k = topk_idx.shape[1]
    if k == 0:
        return full_order
    perm = torch.sort(itm_scores, dim=1, descending=True, stable=True).indices
    return torch.cat((torch.gather(topk_idx.long(), 1, perm), full_order[:, k:]), dim=1)


def itc_order(sim):
    """Ranking of every row of `sim` by similarity descending, equal values by ascending index (the order ops.topk_rows cuts its k from)."""
    return torch.sort(sim, dim=1, descending=True, stable=True).indices


@torch.no_grad()
def rerank_retrieval(model, feat_t, input_ids, attention_mask, feat_cond, condition_feats, k=None, directions=("t2c", "c2t"),
                     kv_budget_bytes=None, pair_batch=512, trim_text=True):
    """ITC shortlist + ITM re-ranking.  feat_t [Nq, C], feat_cond [Nc, C]: the normalised contrastive features; input_ids /
    attention_mask [Nq, S]; condition_feats [Nc, E, D].  k: shortlist length (None: model.config.itm_rerank_num, else 50; cut to the
    number of columns and to ops.TOPK_MAX); k = 0 skips ITM.  Returns {direction: {"topk_idx" int64, "itc_scores", "itm_scores" (each
    [rows, k]), "order" int64 [rows, cols]}} - rows are texts and columns candidates for "t2c", the reverse for "c2t"."""
    for d in directions:
        if d not in ("t2c", "c2t"):
            raise ValueError(f"unknown direction {d!r}")
    if k is None:
        cfg = getattr(model, "config", None)
        k = cfg.get("itm_rerank_num") if cfg is not None and hasattr(cfg, "get") else None
        k = 50 if k is None else k
    k = int(k)
    dev = feat_t.device
    feat_t, feat_cond = feat_t.float().contiguous(), feat_cond.float().contiguous()
    Nq, Nc = feat_t.shape[0], feat_cond.shape[0]
    sim = Fn.matmul_nt(feat_t, feat_cond)                          # [Nq, Nc]; the other direction ranks the same numbers
    sims = {"t2c": sim, "c2t": sim.t().contiguous() if "c2t" in directions else None}
    out, tops = {}, {"t2c": None, "c2t": None}
    for d in directions:
        s = sims[d]
        kd = min(k, s.shape[1], ops.TOPK_MAX)
        if kd > 0:
            val, idx = ops.topk_rows(s, kd)
        else:
            val, idx = s.new_empty((s.shape[0], 0)), torch.empty((s.shape[0], 0), dtype=torch.int32, device=dev)
        out[d] = dict(topk_idx=idx.long(), itc_scores=val, itm_scores=s.new_empty((s.shape[0], kd)))
        tops[d] = idx.cpu() if kd > 0 else None
    if any(t is not None for t in tops.values()):
        plan = plan_pairs(tops["t2c"], tops["c2t"], n_text=Nq, n_cand=Nc)      # on the host: the index tables are built without a device sync per chunk
        scores = score_pairs(model, input_ids, attention_mask, condition_feats, plan, kv_budget_bytes, pair_batch, trim_text)
        for d, inv in (("t2c", plan.inv_t2c), ("c2t", plan.inv_c2t)):
            if inv is not None:
                out[d]["itm_scores"] = scores[inv.to(dev)]
        out["plan"] = plan
    for d in directions:
        out[d]["order"] = compose_order(out[d]["topk_idx"], out[d]["itm_scores"], itc_order(sims[d]))
    return out


def _ranks(order):
    """pos[i, c] = position of column c in the ranking order[i]."""
    pos = torch.empty_like(order)
    pos.scatter_(1, order, torch.arange(order.shape[1], device=order.device).unsqueeze(0).expand_as(order))
    return pos


def retrieval_metrics(order_t2c, order_c2t, text_to_cond):
    """R@1 / R@5 / R@10 (percent) and the median rank (1-based) of both directions.  order_t2c [Nq, Nc] / order_c2t [Nc, Nq]: final rankings
    (either may be None); text_to_cond [Nq]: the candidate every text belongs to.  A candidate with several captions is a hit in c2t when
    any of its texts is within the cut (its rank is that of its best-ranked text); candidates without a text are left out."""
    t2c = torch.as_tensor(text_to_cond, dtype=torch.long)
    out = {}

    def put(name, rank):
        rank = rank.double()
        for r in (1, 5, 10):
            out[f"{name}_r{r}"] = float((rank < r).double().mean() * 100.0) if rank.numel() else float("nan")
        out[f"{name}_medr"] = float(rank.median() + 1) if rank.numel() else float("nan")

    if order_t2c is not None:
        o = order_t2c.cpu().long()
        put("t2c", _ranks(o).gather(1, t2c.view(-1, 1)).view(-1))
    if order_c2t is not None:
        o = order_c2t.cpu().long()
        pos = _ranks(o)                                              # [Nc, Nq]
        r_text = pos[t2c, torch.arange(t2c.numel())]                 # rank of text i in its own candidate's row
        best = torch.full((o.shape[0],), o.shape[1], dtype=torch.long).scatter_reduce(0, t2c, r_text, reduce="amin")
        has = torch.zeros(o.shape[0], dtype=torch.bool).index_fill_(0, t2c, True)
        put("c2t", best[has])
    return out


class RetrievalEvaluator:
    """Accumulates the evaluation dictionaries of `MiCo.forward(batch, "ret%<subtask>", compute_loss=False)` over a test set and scores it.
    Features are kept in fp32, the condition tokens in the 16-bit compute dtype (the bulk of the memory), all on the device they arrive on."""

    def __init__(self, model, subtask):
        self.model, self.subtask = model, subtask
        self.feat_t, self.ids, self.mask, self.feat_c, self.cond, self.t2c = [], [], [], [], [], []
        self.n_cand = 0

    def add(self, eval_dict, text_to_cond=None):
        """text_to_cond: for every text of this batch the number of its candidate WITHIN this batch (None: text i belongs to candidate i)."""
        fc = eval_dict[f"feat_cond_{self.subtask}"]
        nt = eval_dict["feat_t"].shape[0]
        if text_to_cond is None:
            if nt != fc.shape[0]:
                raise ValueError("text_to_cond is needed when a batch has not one text per candidate")
            text_to_cond = torch.arange(nt)
        t2c = torch.as_tensor(text_to_cond, dtype=torch.long).cpu()
        if t2c.numel() != nt or (nt and (int(t2c.min()) < 0 or int(t2c.max()) >= fc.shape[0])):
            raise ValueError("text_to_cond names a candidate of this batch for every text")
        self.feat_t.append(eval_dict["feat_t"].detach().float())
        self.ids.append(eval_dict["input_ids"])
        self.mask.append(eval_dict["attention_mask"])
        self.feat_c.append(fc.detach().float())
        self.cond.append(eval_dict[f"condition_feats_{self.subtask}"].detach().to(runtime.compute_dtype()))
        self.t2c.append(t2c + self.n_cand)
        self.n_cand += fc.shape[0]

    def finish(self, k=None, **kw):
        """{"metrics": retrieval_metrics(...), "t2c": tables, "c2t": tables}; kw goes to rerank_retrieval."""
        t2c = torch.cat(self.t2c)
        res = rerank_retrieval(self.model, torch.cat(self.feat_t), torch.cat(self.ids), torch.cat(self.mask), torch.cat(self.feat_c),
                               torch.cat(self.cond), k=k, **kw)
        res["metrics"] = retrieval_metrics(res["t2c"]["order"] if "t2c" in res else None, res["c2t"]["order"] if "c2t" in res else None, t2c)
        res["text_to_cond"] = t2c
        return res
