"""Argument checks of the incremental caption decode (BertForMaskedLM.generate(use_cache=True), ops.attn_decode) that need no GPU."""
import pytest
import torch

from mico_amd import ops
from mico_amd.model.bert import BertForMaskedLM

_SMALL = dict(num_hidden_layers=1, vocab_size=128, intermediate_size=64)


def test_use_cache_refuses_training_mode():
    m = BertForMaskedLM(_SMALL).train()
    ids = torch.full((1, 1), 101)
    with pytest.raises(RuntimeError, match="inference-only"):
        m.generate(input_ids=ids, attention_mask=ids.new_ones(1, 1, 1), max_new_tokens=2, use_cache=True)


def test_num_return_sequences_needs_sampling():
    m = BertForMaskedLM(_SMALL).eval()
    ids = torch.full((1, 1), 101)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(input_ids=ids, attention_mask=ids.new_ones(1, 1, 1), max_new_tokens=2, num_beams=3, num_return_sequences=2)


def test_attn_decode_refuses_other_head_sizes_before_any_launch():
    q = torch.zeros(2, 128, dtype=torch.float16)      # host tensors: a launch would fail differently
    with pytest.raises(ops.MicoHipError, match="hd 64 only"):
        ops.attn_decode(q, q, q, q, sets=1, rows_per_set=1, q_per_row=2, H=4, Sk=2, hd=32, scale=1.0, q_rs=128, kv_strides=(256, 128),
                        o_rs=128)
