"""Patch dropout (FLIP) in the EVA towers, host side (no GPU): the public surface (create_model(force_patch_dropout), the MiCo
`patch_dropout` key, visual.patch_dropout's shape), the keep-count formula, the host draw against the reference's own draw recorded in
tests/golden/patch_dropout_*.pt, validation of injected tables, and the towers that refuse the option."""
import pytest
import torch
from torch import nn

from common import golden, build_model
from mico_amd import functional as Fn
from mico_amd.model.evaclip import PatchDropout, create_model


class _Captured(Exception):
    pass


@pytest.fixture
def capture_tower(monkeypatch):
    """Replaces the device pass (EvaTowerFn.apply) by a recorder: what forward_groups hands to the engine, without a GPU."""
    seen = {}

    def fake_apply(spec, groups, dp_scale, keep, *params):
        seen.update(spec=spec, groups=groups, dp_scale=dp_scale, keep=keep)
        raise _Captured()

    monkeypatch.setattr(Fn.EvaTowerFn, "apply", fake_apply)
    return seen


def test_force_patch_dropout_sets_the_rate():
    vis = create_model("EVA02-CLIP-B-16", layers=1, force_patch_dropout=0.5).visual
    assert isinstance(vis.patch_dropout, PatchDropout)
    assert vis.patch_dropout.prob == 0.5 and vis.patch_dropout.exclude_first_token is True
    assert not list(vis.patch_dropout.parameters())
    assert isinstance(create_model("EVA02-CLIP-B-16", layers=1, force_patch_dropout=0.).visual.patch_dropout, nn.Identity)
    assert isinstance(create_model("EVA02-CLIP-B-16", layers=1).visual.patch_dropout, nn.Identity)


def test_mico_config_key():
    m, _ = build_model("evaclip02_base", 1, patch_dropout=0.75)
    assert m.vision_encoder.visual.patch_dropout.prob == 0.75
    m0, _ = build_model("evaclip02_base", 1)
    assert isinstance(m0.vision_encoder.visual.patch_dropout, nn.Identity)


@pytest.mark.parametrize("np_,p,keep", [(256, 0.5, 128), (256, 0.75, 64), (196, 0.5, 98), (196, 0.75, 49), (256, 0.1, 230), (196, 0.3, 137),
                                        (256, 0.99, 2), (4, 0.9, 1), (1, 0.5, 1), (256, 0.0, 256)])
def test_keep_count(np_, p, keep):
    assert Fn.patch_keep_count(np_, p) == keep == max(1, int(np_ * (1 - p)))


@pytest.mark.parametrize("tag,name", [("b16_d2_p50", "EVA02-CLIP-B-16"), ("g14_d2_p50", "EVA01-CLIP-g-14"), ("g14_d2_p75", "EVA01-CLIP-g-14")])
def test_host_draw_equals_the_reference(tag, name, capture_tower):
    """Under the fixture's seed one tower call draws exactly the reference's kept indices (topk order, unsorted), and the DropPath
    multipliers come after that draw."""
    fx = golden(f"patch_dropout_{tag}.pt")
    vis = create_model(name, layers=2, force_patch_dropout=fx["meta"]["prob"]).visual.train()
    for blk in vis.blocks:
        blk.drop_path_prob = 0.1
    x = torch.zeros(2, 3, 224, 224)
    torch.manual_seed(fx["meta"]["draw_seed"])
    with pytest.raises(_Captured):
        vis.forward_groups([x])
    keep = capture_tower["keep"]
    assert torch.equal(keep.host, fx["keep"])
    assert keep.N == fx["out"].shape[1] and keep.k == fx["keep"].shape[1]
    # the stochastic-depth draw follows the patch draw
    torch.manual_seed(fx["meta"]["draw_seed"])
    torch.randn(2, vis.patch_embed.num_patches)
    assert torch.equal(capture_tower["dp_scale"], vis._drop_path_scale(2, "cpu"))


def test_draw_follows_training_mode_not_grad_mode(capture_tower):
    vis = create_model("EVA02-CLIP-B-16", layers=1, force_patch_dropout=0.5).visual
    x = torch.zeros(3, 3, 224, 224)
    vis.eval()
    with pytest.raises(_Captured):
        vis.forward_groups([x])
    assert capture_tower["keep"] is None
    vis.train()
    with torch.no_grad(), pytest.raises(_Captured):
        vis.forward_groups([x, x[:1]])
    assert capture_tower["keep"].host.shape == (4, 98)      # one draw over all frames of the call
    vis0 = create_model("EVA02-CLIP-B-16", layers=1).visual.train()
    with pytest.raises(_Captured):
        vis0.forward_groups([x])
    assert capture_tower["keep"] is None


def test_invalid_injected_tables_raise(capture_tower):
    vis = create_model("EVA02-CLIP-B-16", layers=1, force_patch_dropout=0.5).visual.train()
    x = torch.zeros(2, 3, 224, 224)
    good = torch.stack([torch.randperm(196)[:98] for _ in range(2)])
    with pytest.raises(_Captured):
        vis.forward_groups([x], patch_keep=good)
    assert torch.equal(capture_tower["keep"].host, good)
    bad_range = good.clone()
    bad_range[1, 5] = 196
    bad_neg = good.clone()
    bad_neg[0, 0] = -1
    bad_repeat = good.clone()
    bad_repeat[0, 1] = bad_repeat[0, 0]
    for bad in (good[:, :97], torch.cat((good, good[:, :1]), 1), good[:1], bad_range, bad_neg, bad_repeat, good.float()):
        with pytest.raises(ValueError):
            vis.forward_groups([x], patch_keep=bad)
    vis0 = create_model("EVA02-CLIP-B-16", layers=1).visual.train()
    with pytest.raises(ValueError):
        vis0.forward_groups([x], patch_keep=good)


def test_swin_refuses_patch_dropout():
    from mico_amd.model import MiCo, default_cfg
    with pytest.raises(ValueError):
        MiCo(default_cfg("swin_tiny_test", patch_dropout=0.5))


def test_postnorm_tower_refuses_patch_dropout(capture_tower):
    vis = create_model("EVA02-CLIP-bigE-14-plus", layers=1, force_patch_dropout=0.5).visual.train()
    with pytest.raises(NotImplementedError):
        vis.forward_groups([torch.zeros(1, 3, 224, 224)])
    vis.eval()       # inactive: the tower runs as before
    with pytest.raises(_Captured):
        vis.forward_groups([torch.zeros(1, 3, 224, 224)])


@pytest.mark.parametrize("vtype", ["evaclip02_base", "evaclip01_giant"])
def test_state_dict_keys_unchanged(vtype):
    from mico_amd.model import MiCo, default_cfg
    ref = golden("state_dict_keys.pt")[vtype]
    with torch.device("meta"):
        on = MiCo(default_cfg(vtype, vision_layers=None, patch_dropout=0.5))
        off = MiCo(default_cfg(vtype, vision_layers=None))
    assert isinstance(on.vision_encoder.visual.patch_dropout, PatchDropout)
    k_on = {k: tuple(v.shape) for k, v in on.state_dict().items()}
    assert k_on == {k: tuple(v.shape) for k, v in off.state_dict().items()}
    for k, (shape, is_param) in ref.items():
        if is_param:
            assert k_on.get(k) == tuple(shape), k
