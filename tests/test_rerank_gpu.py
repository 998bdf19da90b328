"""Retrieval evaluation on the GPU: the indexed-K/V attention forward (bit-exact against a gather), mico_topk_rows against torch.topk on
the CPU, mico_amd.evaluation.rerank_retrieval against the CPU oracle pair by pair, and inference_demo.py --rerank against the default path.

Measured on an MI355X - worst rel_err of an ITM score table against the oracle: fp16 1.7e-4 (bound 2e-3), bf16 2.2e-3 (bound 2.4e-2), the
same with trimmed and with padded text rows; --rerank against the demo's default path: 0 (bit-identical).  DESIGN.md section 7."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from common import build_model, rel_err

pytestmark = pytest.mark.gpu

ITM_TOL = {torch.float16: 2e-3}                               # the bound tests/test_inference_demo_gpu.py holds itm_scores to
ITM_TOL[torch.bfloat16] = ITM_TOL[torch.float16] * (1.2e-2 / 1e-3)      # x the bf16 / fp16 ratio of FWD_TOL in tests/test_model_gpu.py


# ----------------------------------------------------------------------------------------------------------------------
# indexed forward
# ----------------------------------------------------------------------------------------------------------------------
def _attn_pair(cuda, dtype, Sq, Sk, masked, drop=None, seed=0):
    """(o, lse) of ops.attn_fwd reading K/V by index, and of the same call on K/V gathered per batch entry."""
    from mico_amd import ops
    H, hd, D = 12, 64, 768
    sets = 5
    idx = torch.tensor([3, 0, 3, 3, 1, 0, 4, 1, 3], dtype=torch.int32)       # repeats; set 2 is read by nobody
    B = idx.numel()
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B * Sq, D, generator=g).to(dtype).to(cuda)
    kv = torch.randn(sets * Sk, 2 * D, generator=g).to(dtype).to(cuda)
    mask = None
    if masked:
        mask = ((torch.rand(B, Sk, generator=g) < 0.3).float() * -10000.0)
        mask[:, 0] = 0.0
        mask = mask.to(cuda)
    st = dict(B=B, H=H, Sq=Sq, Sk=Sk, hd=hd, scale=hd ** -0.5, mask=mask, q_strides=(Sq * D, D), k_strides=(Sk * 2 * D, 2 * D),
              v_strides=(Sk * 2 * D, 2 * D), o_strides=(Sq * D, D), drop=drop)
    res = []
    for indexed in (True, False):
        o = torch.zeros(B * Sq, D, dtype=dtype, device=cuda)
        lse = torch.zeros(B, H, Sq, dtype=torch.float32, device=cuda)
        if indexed:
            ops.attn_fwd(q, kv, kv[:, D:], o, lse, kv_index=idx.to(cuda), **st)
        else:
            kvg = kv.view(sets, Sk, 2 * D)[idx.long().to(cuda)].reshape(B * Sk, 2 * D).contiguous()
            ops.attn_fwd(q, kvg, kvg[:, D:], o, lse, **st)
        res.append((o, lse))
    torch.cuda.synchronize()
    return res, idx


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Sq,Sk", list(itertools.product((16, 32, 77), (77, 1285))))
def test_indexed_forward_is_the_gathered_forward(cuda, dtype, masked, Sq, Sk):
    ((o1, l1), (o2, l2)), idx = _attn_pair(cuda, dtype, Sq, Sk, masked)
    assert torch.isfinite(o1.float()).all() and torch.isfinite(l1).all() and o1.float().abs().max() > 0
    assert torch.equal(o1, o2) and torch.equal(l1, l2)          # the same kernel reading the same values
    # the index is honoured, not ignored: entries 0 and 2 read the same set with different queries, entries 0 and 1 different sets
    o = o1.view(idx.numel(), Sq, -1)
    assert not torch.equal(o[0], o[1]) and not torch.equal(o[0], o[2])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_indexed_forward_with_dropout_kernel(cuda, dtype):
    """Every instantiation of the tiled kernel honours the table - also the five-wave dropout form BERT's 77 rows take in training (the dropout
    counters are per batch entry, so the gathered call draws the same masks)."""
    ((o1, l1), (o2, l2)), _ = _attn_pair(cuda, dtype, 77, 77, True, drop=(0.1, 1234, 3))
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    ((o1, l1), (o2, l2)), _ = _attn_pair(cuda, dtype, 32, 1285, False, drop=(0.1, 99, 4))
    assert torch.equal(o1, o2) and torch.equal(l1, l2)


def test_indexed_forward_refusals(cuda):
    """Error codes only - nothing is launched: kv_index + kv_batch_mod, and kv_index in the backward."""
    from mico_amd import ops
    from mico_amd._lib import MicoHipError
    B, H, hd, D, Sq, Sk = 4, 12, 64, 768, 16, 77
    q = torch.zeros(B * Sq, D, dtype=torch.float16, device=cuda)
    kv = torch.zeros(2 * Sk, 2 * D, dtype=torch.float16, device=cuda)
    o = torch.zeros_like(q)
    lse = torch.zeros(B, H, Sq, device=cuda)
    idx = torch.zeros(B, dtype=torch.int32, device=cuda)
    st = dict(B=B, H=H, Sq=Sq, Sk=Sk, hd=hd, scale=0.125, q_strides=(Sq * D, D), k_strides=(Sk * 2 * D, 2 * D), v_strides=(Sk * 2 * D, 2 * D),
              o_strides=(Sq * D, D))
    with pytest.raises(MicoHipError, match="kv_index"):
        ops.attn_fwd(q, kv, kv[:, D:], o, lse, kv_index=idx, kv_batch_mod=2, **st)
    with pytest.raises(MicoHipError, match="kv_index"):
        ops.attn_bwd(q, kv, kv[:, D:], o, o, lse, q, kv, kv[:, D:], lse, kv_index=idx, **st)
    with pytest.raises(MicoHipError, match="int32"):
        ops.attn_fwd(q, kv, kv[:, D:], o, lse, kv_index=idx.long(), **st)
    with pytest.raises(MicoHipError, match="int32"):
        ops.attn_fwd(q, kv, kv[:, D:], o, lse, kv_index=idx[:2], **st)


# ----------------------------------------------------------------------------------------------------------------------
# top-k
# ----------------------------------------------------------------------------------------------------------------------
def _distinct(rows, cols, seed):
    """Pairwise distinct values: a seeded permutation of an arithmetic sequence (exact in fp32)."""
    g = torch.Generator().manual_seed(seed)
    n = rows * cols
    return ((torch.randperm(n, generator=g).float() - n // 2) * 0.25).view(rows, cols)


@pytest.mark.parametrize("rows,cols", [(7, 50), (64, 1000), (3, 20000)])
@pytest.mark.parametrize("k", [1, 50, 128])
def test_topk_rows_matches_torch(cuda, rows, cols, k):
    from mico_amd import ops
    if k > cols:
        k = cols                      # the 50-column shape: k <= cols
    x = _distinct(rows, cols, rows * 1000 + k)
    val, idx = ops.topk_rows(x.to(cuda), k)
    rv, ri = torch.topk(x, k, dim=1)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32
    assert torch.equal(idx.cpu().long(), ri)
    assert torch.equal(val.cpu(), rv)         # bit-equal


def test_topk_rows_ties_orders_and_strides(cuda):
    from mico_amd import ops
    from mico_amd._lib import MicoHipError
    x = torch.zeros(4, 300)
    x[:, 250] = 1.0
    x[:, 7] = 1.0
    x[:, 100] = 1.0
    x[3, 0] = -0.0                             # -0 ties with +0: the lower column still wins
    val, idx = ops.topk_rows(x.to(cuda), 6)
    assert idx.cpu().tolist() == [[7, 100, 250, 0, 1, 2]] * 4          # equal values: the lower column first
    assert val.cpu().tolist() == [[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]] * 4
    # rows already sorted: ascending (every element beats the running k-th best: the fold path at its busiest) and descending
    n = 20000
    asc = torch.arange(n, dtype=torch.float32).view(1, n)
    both = torch.cat((asc, asc.flip(1)), 0)
    val, idx = ops.topk_rows(both.to(cuda), 128)
    assert idx[0].cpu().tolist() == list(range(n - 1, n - 129, -1)) and idx[1].cpu().tolist() == list(range(128))
    assert torch.equal(val.cpu(), torch.topk(both, 128, dim=1).values)
    # a column slice of a wider matrix (row stride > cols), -inf entries, k == cols
    wide = _distinct(9, 96, 5)
    wide[2, 3] = float("-inf")
    val, idx = ops.topk_rows(wide.to(cuda)[:, :70], 70)
    rv, ri = torch.topk(wide[:, :70], 70, dim=1)
    assert torch.equal(idx.cpu().long(), ri) and torch.equal(val.cpu(), rv)
    for bad_k in (0, 129, 71):
        with pytest.raises(MicoHipError):
            ops.topk_rows(wide.to(cuda)[:, :70], bad_k)
    with pytest.raises(MicoHipError):
        ops.topk_rows(wide, 3)                 # a CPU tensor: no fallback


# ----------------------------------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------------------------------
NQ, NC, E_TOK, K, S = 12, 6, 2 * 197, 3, 48


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    feat_t = F.normalize(torch.randn(NQ, 512, generator=g), dim=-1)
    feat_c = F.normalize(torch.randn(NC, 512, generator=g), dim=-1)
    cond = torch.randn(NC, E_TOK, 768, generator=g)
    lens = [5, 9, 12, 16, 17, 20, 23, 26, 30, 31, 33, 40]                  # mixed lengths: sub-batches trim to 16 .. 48
    perm = torch.randperm(NQ, generator=g).tolist()
    ids = torch.zeros(NQ, S, dtype=torch.long)
    am = torch.zeros(NQ, S, dtype=torch.long)
    for row, n in zip(perm, lens):
        ids[row, 0] = 101
        ids[row, 1:n - 1] = torch.randint(1000, 30000, (n - 2,), generator=g)
        ids[row, n - 1] = 102
        am[row, :n] = 1
    return feat_t, feat_c, cond, ids, am


@pytest.fixture(scope="module")
def model_sd(cuda):
    m, sd = build_model("evaclip02_base", 2, device=cuda)
    return m, sd


@pytest.fixture(scope="module")
def oracle_scores(model_sd):
    """ITM score of EVERY (text, candidate) pair from the fp32 oracle on the CPU: [NQ, NC]."""
    from oracle import mico_oracle as O
    _, sd = model_sd
    _, _, cond, ids, am = _inputs()
    t = torch.arange(NQ).repeat_interleave(NC)
    c = torch.arange(NC).repeat(NQ)
    out = []
    with torch.no_grad():
        for i in range(0, t.numel(), 24):
            seq = O.bert_forward(sd, ids[t[i:i + 24]], am[t[i:i + 24]], cond[c[i:i + 24]])
            out.append(F.softmax(O.itm_head(sd, seq[:, 0]), dim=1)[:, 1])
    return torch.cat(out).view(NQ, NC)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("trim_text", [True, False])
def test_rerank_against_oracle(cuda, model_sd, oracle_scores, dtype, trim_text):
    from mico_amd import runtime, evaluation as Ev
    from mico_amd import functional as Fn
    model, _ = model_sd
    feat_t, feat_c, cond, ids, am = _inputs()
    with runtime.precision(dtype), torch.no_grad():
        res = Ev.rerank_retrieval(model, feat_t.to(cuda), ids.to(cuda), am.to(cuda), feat_c.to(cuda), cond.to(cuda).to(dtype), k=K,
                                  trim_text=trim_text, pair_batch=16)
        sim = Fn.matmul_nt(feat_t.to(cuda), feat_c.to(cuda)).cpu()
    worst = 0.0
    for d, s in (("t2c", sim), ("c2t", sim.t().contiguous())):
        r = res[d]
        rows = s.shape[0]
        tv, ti = torch.topk(s, K, dim=1)
        assert torch.equal(r["topk_idx"].cpu(), ti) and torch.equal(r["itc_scores"].cpu(), tv)
        assert r["itm_scores"].shape == (rows, K) and r["order"].shape == s.shape
        ref = oracle_scores[torch.arange(rows).unsqueeze(1), ti] if d == "t2c" else oracle_scores[ti, torch.arange(rows).unsqueeze(1)]
        e = rel_err(r["itm_scores"], ref)
        worst = max(worst, e)
        print(f"[rerank {dtype} trim={trim_text}] {d}: itm rel_err {e:.3e} (tol {ITM_TOL[dtype]:g})")
        # the final ranking, recomputed from the product's own scores: shortlist by ITM descending (ties: ITC order), then the rest in ITC order
        itm = r["itm_scores"].cpu()
        for row in range(rows):
            short = sorted(range(K), key=lambda j: (-float(itm[row, j]), j))
            head = [int(ti[row, j]) for j in short]
            rest = [int(c) for c in torch.sort(s[row], descending=True, stable=True).indices.tolist() if int(c) not in head]
            assert r["order"][row].cpu().tolist() == head + rest
    assert worst < ITM_TOL[dtype]
    # a pair both directions ask for was scored once: the identical number in both tables
    t2c, c2t = res["t2c"], res["c2t"]
    shared = 0
    for i in range(NQ):
        for r_, c in enumerate(t2c["topk_idx"][i].tolist()):
            lst = c2t["topk_idx"][c].tolist()
            if i in lst:
                shared += 1
                assert t2c["itm_scores"][i, r_].item() == c2t["itm_scores"][c, lst.index(i)].item()
    assert shared > 0
    assert res["plan"].text.numel() == NQ * K + NC * K - shared
    assert Ev.score_pairs.last_stats["kv_projections"] == len(set(res["plan"].cand.tolist())) <= NC      # every candidate projected once


def test_rerank_chunked_is_bit_identical_and_k0(cuda, model_sd):
    from mico_amd import runtime, evaluation as Ev
    model, _ = model_sd
    feat_t, feat_c, cond, ids, am = _inputs()
    dtype = torch.float16
    args = (model, feat_t.to(cuda), ids.to(cuda), am.to(cuda), feat_c.to(cuda), cond.to(cuda).to(dtype))
    with runtime.precision(dtype), torch.no_grad():
        one = Ev.rerank_retrieval(*args, k=K)
        assert Ev.score_pairs.last_stats["chunks"] == 1
        per_cand = Ev.kv_bytes_per_candidate(E_TOK, 12, 768, 2)
        three = Ev.rerank_retrieval(*args, k=K, kv_budget_bytes=2 * per_cand + 1)        # two candidates per chunk
        assert Ev.score_pairs.last_stats["chunks"] == 3 and Ev.score_pairs.last_stats["max_cands"] == 2
        for d in ("t2c", "c2t"):
            assert torch.equal(one[d]["itm_scores"], three[d]["itm_scores"])
            assert torch.equal(one[d]["order"], three[d]["order"])
        zero = Ev.rerank_retrieval(*args, k=0)
        sim = (feat_t @ feat_c.t())
        assert zero["t2c"]["itm_scores"].shape == (NQ, 0) and "plan" not in zero
        assert zero["t2c"]["order"].cpu().tolist() == torch.sort(sim, dim=1, descending=True, stable=True).indices.tolist()
        # default k: model.config.itm_rerank_num, else 50 - cut to the number of columns
        dflt = Ev.rerank_retrieval(*args, directions=("t2c",))
        assert dflt["t2c"]["itm_scores"].shape == (NQ, NC) and "c2t" not in dflt
    with runtime.precision(dtype):
        with pytest.raises(RuntimeError, match="no_grad"):
            kv = torch.zeros(2, E_TOK, 12 * 2 * 768, dtype=dtype, device=cuda)
            model.multimodal_encoder.bert(input_ids=ids[:2].to(cuda), cross_kv=kv, kv_index=torch.zeros(2, dtype=torch.int32, device=cuda))


def test_evaluator_end_to_end(cuda, model_sd):
    """RetrievalEvaluator over two batches of evaluation dictionaries (as MiCo.forward(..., compute_loss=False) returns them)."""
    from mico_amd import runtime, evaluation as Ev
    model, _ = model_sd
    feat_t, feat_c, cond, ids, am = _inputs()
    t2c = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    with runtime.precision(torch.float16), torch.no_grad():
        ev = Ev.RetrievalEvaluator(model, "tv")
        for b in range(2):
            tq, cq = slice(6 * b, 6 * b + 6), slice(3 * b, 3 * b + 3)
            ev.add({"feat_t": feat_t[tq].to(cuda), "input_ids": ids[tq].to(cuda), "attention_mask": am[tq].to(cuda),
                    "feat_cond_tv": feat_c[cq].to(cuda), "condition_feats_tv": cond[cq].to(cuda)}, [0, 0, 1, 1, 2, 2])
        res = ev.finish(k=K)
        direct = Ev.rerank_retrieval(model, feat_t.to(cuda), ids.to(cuda), am.to(cuda), feat_c.to(cuda), cond.to(cuda).half(), k=K)
    assert res["text_to_cond"].tolist() == t2c
    for d in ("t2c", "c2t"):
        assert torch.equal(res[d]["itm_scores"], direct[d]["itm_scores"]) and torch.equal(res[d]["order"], direct[d]["order"])
    want = Ev.retrieval_metrics(direct["t2c"]["order"], direct["c2t"]["order"], t2c)
    assert res["metrics"] == want and set(want) == {f"{d}_{m}" for d in ("t2c", "c2t") for m in ("r1", "r5", "r10", "medr")}


# ----------------------------------------------------------------------------------------------------------------------
# demo
# ----------------------------------------------------------------------------------------------------------------------
def test_demo_rerank_reproduces_default_itm_scores(cuda, tmp_path):
    import numpy as np
    import inference_demo as demo
    from mico_amd import runtime
    from mico_amd.model import MiCo
    from mico_amd.model.imageprocessor import ImageProcessor
    from PIL import Image
    rng = np.random.RandomState(0)
    path = str(tmp_path / "test.jpeg")
    Image.fromarray((rng.rand(428, 640, 3) * 255).astype(np.uint8)).save(path, quality=95)
    pdir = str(tmp_path / "MiCo-synth")
    demo.write_synthetic_pretrain_dir(pdir, "evaclip02_base", steps=(3, 12), vision_layers=2, max_vision_sample_num=8)
    ckpt, opts = demo.load_from_pretrained_dir(pdir)
    old = runtime.compute_dtype()
    runtime.set_compute_dtype(torch.float16)
    try:
        model = MiCo.from_pretrained(opts, ckpt).to(cuda).eval()
        x = ImageProcessor(224, "swin", training=True)(path)
        texts = ["a man is skiing in a snowy day.", "it's a hot day", "two dogs"]
        base = demo.run_demo(model, x, texts, cuda)
        rer = demo.run_demo(model, x, texts, cuda, rerank=True)
    finally:
        runtime.set_compute_dtype(old)
    e = rel_err(rer["itm_scores"], base["itm_scores"])
    print(f"[demo --rerank] itm rel_err vs default path {e:.3e} (tol 2e-3)")
    assert rer["itm_scores"].shape == base["itm_scores"].shape == (3,)
    assert e < 2e-3
    assert rer["captions"] == base["captions"] and torch.equal(rer["sim_t2v"], base["sim_t2v"])
