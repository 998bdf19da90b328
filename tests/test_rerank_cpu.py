"""Retrieval evaluation, host side (no GPU): the pair planner, the chunker, the composition of the final ranking and the metrics of
mico_amd.evaluation, on hand-built cases with known answers; and the C-ABI surface of the feature (struct field, entry point, version)."""
import ctypes

import pytest
import torch

from mico_amd import evaluation as E


def _tables(seed=0, nq=9, nc=5, k=3):
    g = torch.Generator().manual_seed(seed)
    top_t2c = torch.stack([torch.randperm(nc, generator=g)[:k] for _ in range(nq)])
    top_c2t = torch.stack([torch.randperm(nq, generator=g)[:k] for _ in range(nc)])
    return top_t2c, top_c2t


def test_plan_pairs_union_order_and_inverse_maps():
    nq, nc, k = 9, 5, 3
    top_t2c, top_c2t = _tables(0, nq, nc, k)
    plan = E.plan_pairs(top_t2c, top_c2t)
    pairs = list(zip(plan.text.tolist(), plan.cand.tolist()))
    want = {(i, int(c)) for i in range(nq) for c in top_t2c[i]} | {(int(t), j) for j in range(nc) for t in top_c2t[j]}
    assert len(pairs) == len(set(pairs))                       # every pair once
    assert set(pairs) == want                                  # exactly the union
    assert len(want) < nq * k + nc * k                         # (the case has pairs both directions ask for)
    assert pairs == sorted(pairs, key=lambda p: (p[1], p[0]))  # candidate-major, texts ascending within a candidate
    # a made-up per-pair score that names its pair: the inverse maps rebuild both [., k] tables
    score = plan.text.double() * 1000 + plan.cand.double()
    rows_q = torch.arange(nq).unsqueeze(1).expand(nq, k)
    rows_c = torch.arange(nc).unsqueeze(1).expand(nc, k)
    assert torch.equal(score[plan.inv_t2c], rows_q.double() * 1000 + top_t2c.double())
    assert torch.equal(score[plan.inv_c2t], top_c2t.double() * 1000 + rows_c.double())
    # a pair both directions ask for is one entry: both tables point at the same pair number
    both = {(i, int(c)) for i in range(nq) for c in top_t2c[i]} & {(int(t), j) for j in range(nc) for t in top_c2t[j]}
    assert both
    for i, c in both:
        r1 = top_t2c[i].tolist().index(c)
        r2 = top_c2t[c].tolist().index(i)
        assert plan.inv_t2c[i, r1] == plan.inv_c2t[c, r2]


def test_plan_pairs_one_direction_and_int32_tables():
    top_t2c, top_c2t = _tables(1)
    p = E.plan_pairs(top_t2c.int(), None, n_cand=5)
    assert p.inv_c2t is None and p.text.numel() == top_t2c.numel()
    assert torch.equal(p.cand[p.inv_t2c], top_t2c)
    p = E.plan_pairs(None, top_c2t.int(), n_text=9)
    assert p.inv_t2c is None and torch.equal(p.text[p.inv_c2t], top_c2t)
    with pytest.raises(ValueError):
        E.plan_pairs(None, None)
    with pytest.raises(ValueError):
        E.plan_pairs(torch.tensor([[7]]), None, n_cand=5)


@pytest.mark.parametrize("max_cands", [1, 2, 3, 100])
def test_chunks_never_split_a_candidate(max_cands):
    top_t2c, top_c2t = _tables(2, nq=12, nc=7, k=3)
    plan = E.plan_pairs(top_t2c, top_c2t)
    chunks = E.plan_chunks(plan.cand, max_cands)
    seen, pos = [], 0
    for cands, p0, p1, kv_index in chunks:
        assert p0 == pos and p1 > p0 and 1 <= cands.numel() <= max_cands
        pos = p1
        assert kv_index.dtype == torch.int32 and kv_index.numel() == p1 - p0
        assert int(kv_index.min()) >= 0 and int(kv_index.max()) < cands.numel()       # the table the kernel trusts
        assert torch.equal(cands[kv_index.long()], plan.cand[p0:p1])                 # ... names each pair's candidate
        seen += cands.tolist()
    assert pos == plan.cand.numel()
    assert seen == sorted(set(plan.cand.tolist()))          # every candidate with a pair in exactly one chunk
    assert len(chunks) == -(-len(seen) // max_cands)
    with pytest.raises(ValueError):
        E.plan_chunks(plan.cand, 0)


def test_trimmed_length():
    am = torch.zeros(3, 77, dtype=torch.long)
    am[0, :5] = 1
    am[1, :17] = 1
    assert E.trimmed_length(am[:1]) == 16
    assert E.trimmed_length(am) == 32
    am[2, :70] = 1
    assert E.trimmed_length(am) == 77          # never beyond the padded length
    am[0, 40] = 1                              # a hole in the mask: the last attended position counts
    assert E.trimmed_length(am[:1]) == 48


# 6 texts x 4 candidates: candidates 0, 1, 2 have two captions each, candidate 3 none; text i belongs to candidate T2C[i]
T2C = [0, 1, 2, 0, 1, 2]


def _case():
    # ITC similarity with known rows (distinct values per row)
    sim = torch.tensor([[0.9, 0.1, 0.2, 0.3],      # text 0 (cand 0): ITC rank of its own = 0
                        [0.5, 0.4, 0.6, 0.1],      # text 1 (cand 1): own third (rank 2)
                        [0.1, 0.2, 0.3, 0.4],      # text 2 (cand 2): own second (rank 1)
                        [0.2, 0.8, 0.1, 0.3],      # text 3 (cand 0): own third (rank 2)
                        [0.3, 0.9, 0.2, 0.1],      # text 4 (cand 1): own first
                        [0.4, 0.3, 0.2, 0.1]])     # text 5 (cand 2): own third (rank 2)
    return sim


def test_order_k0_is_the_itc_ranking_and_metrics():
    sim = _case()
    o_t2c = E.compose_order(torch.empty(6, 0, dtype=torch.long), torch.empty(6, 0), E.itc_order(sim))
    assert o_t2c.tolist() == [[0, 3, 2, 1], [2, 0, 1, 3], [3, 2, 1, 0], [1, 3, 0, 2], [1, 0, 2, 3], [0, 1, 2, 3]]
    o_c2t = E.compose_order(torch.empty(4, 0, dtype=torch.long), torch.empty(4, 0), E.itc_order(sim.t().contiguous()))
    assert o_c2t.tolist() == [[0, 1, 5, 4, 3, 2], [4, 3, 1, 5, 2, 0], [1, 2, 0, 4, 5, 3], [2, 0, 3, 1, 4, 5]]
    m = E.retrieval_metrics(o_t2c, o_c2t, T2C)
    # t2c ranks of the own candidate: [0, 2, 1, 2, 0, 2]
    assert m["t2c_r1"] == pytest.approx(100 * 2 / 6) and m["t2c_r5"] == 100.0 and m["t2c_r10"] == 100.0
    assert m["t2c_medr"] == 2.0      # ranks sorted [0, 0, 1, 2, 2, 2]: the lower middle (torch.median) is 1 -> 1-based 2
    # c2t: cand 0 has texts {0, 3}: positions 0 and 4 -> 0;  cand 1 has {1, 4}: positions 2 and 0 -> 0;  cand 2 has {2, 5}: 1 and 4 -> 1;  cand 3: none
    assert m["c2t_r1"] == pytest.approx(100 * 2 / 3) and m["c2t_r5"] == 100.0
    assert m["c2t_medr"] == 1.0


def test_order_composition_with_rerank_and_ties():
    sim = _case()
    full = E.itc_order(sim)
    k = 2
    topk = full[:, :k]
    # ITM prefers the second shortlisted candidate in rows 0 and 1, ties in row 2 (ITC order stays), keeps the rest
    itm = torch.tensor([[0.1, 0.9], [0.2, 0.7], [0.5, 0.5], [0.9, 0.1], [0.6, 0.3], [0.8, 0.2]])
    order = E.compose_order(topk, itm, full)
    assert order.tolist() == [[3, 0, 2, 1], [0, 2, 1, 3], [3, 2, 1, 0], [1, 3, 0, 2], [1, 0, 2, 3], [0, 1, 2, 3]]
    for r in range(6):
        assert sorted(order[r].tolist()) == [0, 1, 2, 3]
    m = E.retrieval_metrics(order, None, T2C)
    # own candidates [0, 1, 2, 0, 1, 2] now at ranks [1, 2, 1, 2, 0, 2]
    assert m["t2c_r1"] == pytest.approx(100 / 6) and "c2t_r1" not in m
    assert m["t2c_medr"] == 2.0      # sorted ranks [0, 1, 1, 2, 2, 2]: lower middle 1 -> 1-based 2


def test_two_captions_any_hit_counts():
    # candidate 0 with captions {0, 1}: text 1 is ranked first for it, text 0 last -> a hit at 1
    order_c2t = torch.tensor([[1, 2, 3, 0], [2, 3, 0, 1]])
    m = E.retrieval_metrics(None, order_c2t, [0, 0, 1, 1])
    # cand 0: best of positions (3, 0) = 0;  cand 1: texts {2, 3} at positions (0, 1) -> 0
    assert m["c2t_r1"] == 100.0 and m["c2t_medr"] == 1.0
    m = E.retrieval_metrics(None, torch.tensor([[2, 3, 1, 0], [0, 1, 2, 3]]), [0, 0, 1, 1])
    # cand 0: texts {0, 1} at positions (3, 2) -> 2;  cand 1: texts {2, 3} at (2, 3) -> 2
    assert m["c2t_r1"] == 0.0 and m["c2t_r5"] == 100.0 and m["c2t_medr"] == 3.0


def test_evaluator_accumulates_offsets_cpu():
    """RetrievalEvaluator.add keeps fp32 features, 16-bit condition tokens and global candidate numbers (no model is touched before finish)."""
    from mico_amd import runtime
    ev = E.RetrievalEvaluator(model=None, subtask="tv")
    for n_t, n_c, t2c in ((4, 2, [0, 0, 1, 1]), (3, 3, None)):
        d = {"feat_t": torch.randn(n_t, 8, dtype=torch.float64), "input_ids": torch.ones(n_t, 5, dtype=torch.long),
             "attention_mask": torch.ones(n_t, 5, dtype=torch.long), "feat_cond_tv": torch.randn(n_c, 8),
             "condition_feats_tv": torch.randn(n_c, 6, 16)}
        ev.add(d, t2c)
    assert torch.cat(ev.t2c).tolist() == [0, 0, 1, 1, 2, 3, 4]
    assert ev.feat_t[0].dtype == torch.float32 and ev.cond[0].dtype == runtime.compute_dtype() and ev.cond[0].element_size() == 2
    with pytest.raises(ValueError):
        ev.add({"feat_t": torch.randn(3, 8), "input_ids": None, "attention_mask": None, "feat_cond_tv": torch.randn(2, 8),
                "condition_feats_tv": torch.randn(2, 6, 16)}, None)


def test_abi_has_the_indexed_kv_field_and_topk_entry_point():
    """kv_index is the LAST field of mico_attn_params in the header, the ctypes mirror and the compiled layout; mico_topk_rows is exported;
    its argument checks are host code (no launch): k outside [1, 128] or above cols is MICO_EINVAL."""
    from mico_amd import _lib
    assert _lib.AttnParams._fields_[-1] == ("kv_index", ctypes.c_void_p)
    l = _lib.lib()
    assert l.mico_version() == _lib.ABI_VERSION >= 117
    assert "mico_topk_rows" in _lib.PROTOTYPES
    fake = ctypes.c_void_p(4096)      # never dereferenced: the checks fail before any launch
    for cols, k in ((50, 0), (50, 129), (50, 51), (1000, -1)):
        assert l.mico_topk_rows(fake, cols, 4, cols, k, fake, fake, None) == -22
    assert l.mico_topk_rows(fake, 10, 4, 50, 5, fake, fake, None) == -22        # row stride below cols
    assert l.mico_topk_rows(None, 50, 4, 50, 5, fake, fake, None) == -22
    assert b"mico_topk_rows" in l.mico_last_error_string()


def test_attn_kv_index_error_codes_without_launch():
    """Host-side refusals as return values: kv_index + kv_batch_mod in the forward, any kv_index in the backward.  No kernel runs."""
    from mico_amd import _lib
    l = _lib.lib()
    fake = ctypes.c_void_p(4096)
    p = _lib.AttnParams(B=2, H=12, Sq=16, Sk=77, hd=64, q_bs=16 * 768, q_rs=768, k_bs=77 * 1536, k_rs=1536, v_bs=77 * 1536, v_rs=1536,
                        o_bs=16 * 768, o_rs=768, scale=0.125)
    p.kv_index = 4096
    p.kv_batch_mod = 2
    assert l.mico_attn_fwd(fake, fake, fake, fake, fake, ctypes.byref(p), _lib.F16, None) == -22
    assert b"kv_index" in l.mico_last_error_string()
    p.kv_batch_mod = 0
    assert l.mico_attn_bwd(fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, ctypes.byref(p), _lib.F16, None) == -22
    assert b"kv_index" in l.mico_last_error_string()


def test_bert_kv_index_argument_checks_cpu():
    """BertModel.forward refuses kv_index with grad enabled, without cross_kv, and with a table of the wrong type - before anything runs."""
    from common import build_model
    m, _ = build_model("evaclip02_base", 1)
    bert = m.multimodal_encoder.bert
    ids = torch.ones(2, 4, dtype=torch.long)
    kv = torch.zeros(3, 5, len(bert.encoder.layer) * 2 * 768, dtype=torch.float16)
    idx = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no_grad"):
        bert(input_ids=ids, cross_kv=kv, kv_index=idx)
    with torch.no_grad():
        with pytest.raises(ValueError):
            bert(input_ids=ids, kv_index=idx)
        with pytest.raises(ValueError):
            bert(input_ids=ids, cross_kv=kv, kv_index=idx.long())
        with pytest.raises(ValueError):
            bert(input_ids=ids, cross_kv=kv.view(15, -1), kv_index=idx)          # 2-D memory without kv_sets
