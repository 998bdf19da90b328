"""SCST caption fine-tuning, host side (no GPU): the two-stream builder against a brute-force statement of the [MASK]-append protocol,
MiCo.forward_scst's plumbing over a stub model step, and the C-ABI of the two entry points behind it."""
import ctypes
import os
import re
import types

import pytest
import torch

from mico_amd.model import mico_forward as MF
from mico_amd.model.bert import BertForMaskedLM, first_eos_valid, two_stream_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK, CLS, SEP, PAD = 103, 101, 102, 0


# ---------------------------------------------------------------------------------------------------------------------
# 1. two-stream builder
# ---------------------------------------------------------------------------------------------------------------------
def _grown(mask, L):
    """bert.py:1110-1117 applied until the mask has L positions, entry by entry"""
    while mask.shape[1] < L:
        b, n, _ = mask.shape
        up = torch.zeros(b, n + 1, n + 1, dtype=mask.dtype)
        for r in range(b):
            for i in range(n):
                for j in range(n):
                    up[r, i, j] = mask[r, i, j]
            for j in range(n):
                up[r, n, j] = mask[r, n - 1, j]
            up[r, n, n] = 1
        mask = up
    return mask


def _prompts():
    g = torch.Generator().manual_seed(5)
    cap = (torch.full((3, 1), CLS), torch.ones(3, 1, 1, dtype=torch.long))
    kp = torch.ones(2, 6, dtype=torch.long)
    kp[1, 4:] = 0                                             # one row with 2 padded keys
    q = torch.randint(1000, 30000, (2, 6), generator=g) * kp
    qa = (torch.cat([q, torch.full((2, 1), CLS)], 1), BertForMaskedLM.update_attention_mask(kp[:, None, :].expand(2, 6, 6).contiguous()))
    return {"caption": cap, "question": qa}, g


@pytest.mark.parametrize("kind,P", [("caption", 1), ("question", 7)])
def test_two_stream_builder_states_the_protocol(kind, P):
    prompts, g = _prompts()
    prompt, pmask = prompts[kind]
    T = 4
    assert prompt.shape[1] == P
    R, L = prompt.shape[0], P + T
    ids = torch.cat([prompt, torch.randint(1000, 30000, (R, T), generator=g)], 1)
    G = _grown(pmask, L)
    ids2, m2, pos = two_stream_inputs(ids, pmask, P, MASK)
    S2 = L - 1 + T
    assert ids2.shape == (R, S2) and m2.shape == (R, S2, S2) and pos.shape == (S2,)
    assert torch.equal(ids2[:, :L - 1], ids[:, :L - 1]) and bool((ids2[:, L - 1:] == MASK).all())
    assert pos.tolist() == list(range(L - 1)) + list(range(P, L))
    for r in range(R):
        for i in range(L - 1):                                # token rows: G, and no column of the mask stream
            assert m2[r, i, :L - 1].tolist() == G[r, i, :L - 1].tolist()
            assert m2[r, i, L - 1:].sum() == 0
        for k in range(T):
            t, row = P + k, m2[r, L - 1 + k]
            assert row[:t].tolist() == G[r, t, :t].tolist()   # what the appended [MASK] saw at step t
            assert row[t:L - 1].sum() == 0                    # not token column t (nor a later one)
            for k2 in range(T):                               # itself, no other [MASK]
                assert row[L - 1 + k2] == (1 if k2 == k else 0)
    if kind == "question":                                    # the padded keys stay hidden from every row
        assert m2[1, :, 4:6].sum() == 0
    # the grown mask is accepted as well, and gives the same
    again = two_stream_inputs(ids, G, P, MASK)
    assert all(torch.equal(a, b) for a, b in zip(again, (ids2, m2, pos)))
    with pytest.raises(ValueError):
        two_stream_inputs(ids, pmask[:, :, :1] if P > 1 else torch.ones(R, 2, 2, dtype=torch.long), P, MASK)
    with pytest.raises(ValueError):
        two_stream_inputs(ids[:, :P], pmask, P, MASK)         # nothing generated


def test_first_eos_valid():
    t = torch.tensor([[5, SEP, PAD, PAD], [5, 6, 7, 8], [SEP, PAD, SEP, PAD]])
    assert first_eos_valid(t, SEP).tolist() == [[True, True, False, False], [True] * 4, [True, False, False, False]]
    assert bool(first_eos_valid(t, None).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. forward_scst over a stub model step
# ---------------------------------------------------------------------------------------------------------------------
class _Tok:
    bos_token_id, sep_token_id, pad_token_id, mask_token_id = CLS, SEP, PAD, MASK

    def batch_decode(self, ids, skip_special_tokens=True):
        return [" ".join(f"w{int(t)}" for t in row if int(t) not in (CLS, SEP, PAD)) for row in ids]


class _StubEncoder:
    """scst_rollout returns stored ids, sequence_logprobs a differentiable function of a parameter; both record their calls"""

    def __init__(self, greedy, sampled, T):
        self.tokenizer, self.greedy, self.sampled, self.T = _Tok(), greedy, sampled, T
        self.theta = torch.nn.Parameter(torch.linspace(-1.0, -0.1, sampled.shape[0] * T).view(sampled.shape[0], T))
        self.calls = []

    def scst_rollout(self, prompt, mask, cond, do_sample=True, sample_noise=None, num_return_sequences=1, **kw):
        self.calls.append(("rollout", do_sample, num_return_sequences, sample_noise, kw, cond.requires_grad))
        ids = self.sampled if do_sample else self.greedy
        return torch.cat([prompt.repeat_interleave(num_return_sequences, 0), ids], 1), torch.zeros(ids.shape)

    def sequence_logprobs(self, ids, mask, cond, prompt_len=None, eos_token_id=None, pad_token_id=None):
        self.calls.append(("score", tuple(ids.shape), tuple(mask.shape), tuple(cond.shape), prompt_len, eos_token_id))
        valid = first_eos_valid(ids[:, prompt_len:], eos_token_id)
        return self.theta * valid + 0.0 * cond.sum()


def _stub_model(monkeypatch, b, K, T):
    greedy = torch.tensor([[11, 12, SEP, PAD], [13, SEP, PAD, PAD], [14, 15, 16, 17]])[:b, :T]
    sampled = torch.tensor([[11, SEP, PAD, PAD], [21, 22, 23, SEP], [13, 31, SEP, PAD], [SEP, PAD, PAD, PAD], [14, 15, 16, 17],
                            [41, 42, SEP, PAD]])[:b * K, :T]
    me = _StubEncoder(greedy, sampled, T)
    cond = torch.randn(b, 5, 8, requires_grad=True)
    self = types.SimpleNamespace(multimodal_encoder=me, max_caption_len=T, config={"decode_use_cache": True})
    seen = []
    monkeypatch.setattr(MF, "encode_batch", lambda s, batch: seen.append("encode") or {"condition_feats_v": cond})
    return self, me, cond, seen


def test_forward_scst_plumbing(monkeypatch):
    b, K, T = 3, 2, 4
    self, me, cond, seen = _stub_model(monkeypatch, b, K, T)
    rewards = {"g": [0.5, 0.25, 1.0], "s": [0.75, 0.5, 0.25, 0.0, 1.0, 2.0]}
    got = []

    def reward_fn(captions, sample_index, batch):
        got.append((list(captions), list(sample_index), batch))
        return rewards["g" if len(captions) == b else "s"]

    batch = {"raw_captions": ["a", "b", "c"]}
    noise = torch.rand(b * K, T)
    out = MF.forward_scst(self, batch, "cap%tv", reward_fn, num_samples=K, sample_noise=noise)
    assert set(out) == {"loss_scst", "reward_sample", "reward_greedy", "sampled_captions_tv", "greedy_captions_tv"}
    # one greedy roll-out of b rows, one sampled of b x K (sample-major) with the noise, neither with a gradient; one scoring pass, sampled rows only
    kinds = [c[0] for c in me.calls]
    assert kinds == ["rollout", "rollout", "score"]
    assert me.calls[0][1:3] == (False, 1) and me.calls[1][1:3] == (True, K) and me.calls[1][3] is noise
    assert not me.calls[0][5] and not me.calls[1][5]
    assert me.calls[0][4] == dict(max_new_tokens=T, eos_token_id=SEP, pad_token_id=PAD, use_cache=True)
    assert me.calls[2][1:] == ((b * K, 1 + T), (b * K, 1, 1), (b * K, 5, 8), 1, SEP)
    # reward_fn: the decoded strings and the sample indices, greedy first
    assert got[0][0] == ["w11 w12", "w13", "w14 w15 w16 w17"] and got[0][1] == [0, 1, 2] and got[0][2] is batch
    assert got[1][0] == ["w11", "w21 w22 w23", "w13 w31", "", "w14 w15 w16 w17", "w41 w42"] and got[1][1] == [0, 0, 1, 1, 2, 2]
    assert out["greedy_captions_tv"] == got[0][0] and out["sampled_captions_tv"] == got[1][0]
    # the advantage of row b K + i uses the greedy reward of sample b; valid tokens count the eos
    adv = torch.tensor([0.75 - 0.5, 0.5 - 0.5, 0.25 - 0.25, 0.0 - 0.25, 1.0 - 1.0, 2.0 - 1.0])
    valid = torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 1, 0], [1, 0, 0, 0], [1, 1, 1, 1], [1, 1, 1, 0]], dtype=torch.float32)
    assert valid.sum() == 17
    want = -(adv[:, None] * me.theta.detach() * valid).sum() / 17
    assert torch.allclose(out["loss_scst"], want, rtol=1e-6, atol=0)
    assert abs(float(out["reward_sample"]) - 4.5 / 6) < 1e-6 and abs(float(out["reward_greedy"]) - 1.75 / 3) < 1e-6
    out["loss_scst"].backward()
    assert torch.allclose(me.theta.grad, -(adv[:, None] * valid) / 17, rtol=1e-6, atol=0)
    assert cond.grad is not None                              # the scoring pass reads the condition tokens WITH their graph


def test_forward_scst_averages_sub_tasks_and_takes_noise_per_sub_task(monkeypatch):
    b, K, T = 3, 2, 4
    self, me, cond, _ = _stub_model(monkeypatch, b, K, T)
    noise = {"tv": torch.rand(b * K, T), "tvv": None}
    monkeypatch.setattr(MF, "SUBTASKS", MF.SUBTASKS + ("tvv",))
    monkeypatch.setattr(MF, "_condition_feats", lambda s, enc, key: cond)
    out = MF.forward_scst(self, {}, "cap%tv%tvv", lambda c, i, batch: [float(len(x)) for x in c], num_samples=K, sample_noise=noise)
    assert me.calls[1][3] is noise["tv"] and me.calls[4][3] is None
    one = MF.forward_scst(self, {}, "cap%tv", lambda c, i, batch: [float(len(x)) for x in c], num_samples=K)
    assert torch.allclose(out["loss_scst"], one["loss_scst"])     # two identical sub-tasks: the mean is either
    assert {"sampled_captions_tv", "sampled_captions_tvv", "greedy_captions_tv", "greedy_captions_tvv"} <= set(out)


def test_forward_scst_argument_errors_come_before_any_launch(monkeypatch):
    self, me, cond, seen = _stub_model(monkeypatch, 3, 2, 4)
    fn = lambda c, i, batch: [0.0] * len(c)
    for task in ("ret%tv", "cap", "cap%xx", "cap%tv_ret%tv", "qa%tv"):
        with pytest.raises(ValueError):
            MF.forward_scst(self, {}, task, fn)
    with pytest.raises(TypeError):
        MF.forward_scst(self, {}, "cap%tv", None)
    with pytest.raises(ValueError):
        MF.forward_scst(self, {}, "cap%tv", fn, num_samples=0)
    assert not seen and not me.calls
    with pytest.raises(ValueError, match="rewards"):
        MF.forward_scst(self, {}, "cap%tv", lambda c, i, batch: [0.0], num_samples=2)


def test_forward_scst_is_a_method_and_forward_still_refuses():
    from mico_amd.model.mico import MiCo
    assert MiCo.forward_scst is MF.forward_scst
    assert "qa%" in MF._UNKNOWN_FAMILY or "qa" in MF._UNKNOWN_FAMILY
    # malformed task strings are refused before the model (None) or the batch is touched
    with pytest.raises(ValueError, match="zz"):
        MF.forward(None, {}, "ret%zz")
    with pytest.raises(NotImplementedError, match="forward_qa"):
        MF.forward(None, {}, "foo%tv")


def test_generate_argument_errors():
    """top_k < 0 and a roll-out's argument errors, raised on the host"""
    m = BertForMaskedLM.__new__(BertForMaskedLM)
    torch.nn.Module.__init__(m)
    ids, mask = torch.full((2, 1), CLS), torch.ones(2, 1, 1, dtype=torch.long)
    with pytest.raises(ValueError, match="top_k"):
        m.generate(input_ids=ids, attention_mask=mask, do_sample=True, top_k=-1)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.scst_rollout(ids, mask, None, 3, SEP, PAD, do_sample=False, num_return_sequences=2)
    with pytest.raises(ValueError, match="sample_noise"):
        m.scst_rollout(ids, mask, None, 3, SEP, PAD, sample_noise=torch.rand(2, 4))
    with pytest.raises(ValueError, match="prompt_len"):
        m.sequence_logprobs(ids, mask)


# ---------------------------------------------------------------------------------------------------------------------
# 3. ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_scst_entry_points_declared_exported_and_bound():
    from mico_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mico_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("mico_logprob_fwd_bwd", 13), ("mico_vocab_sample", 11)):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, re.S)
        assert decl, f"{name} is not declared in include/mico_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name])
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.lib().mico_version() == _lib.ABI_VERSION >= 119
    # the entry point INTEGRATION.md's stub binds keeps its 18 arguments
    assert len(_lib.PROTOTYPES["mico_ce_fwd_bwd"]) == 18
