"""crop_flip on the host (no GPU): the sampling plans of mico_amd/model/transforms.py against fixed values and against the independent
restatement in tests/augment_oracle.py, the host paths of ImageProcessor / VideoProcessor against the oracle's torch composition (exact: the
same torch operations), the host-side table validation and the binding of mico_image_augment."""
import os

import numpy as np
import pytest
import torch

import augment_oracle as AO

FALLBACK = {(10, 100): (0, 45, 10, 10), (100, 10): (45, 0, 10, 10), (37, 53): (0, 8, 37, 37), (53, 37): (8, 0, 37, 37),
            (97, 301): (0, 102, 97, 97)}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("size", sorted(FALLBACK))
def test_fallback_boxes_and_draw_count(size):
    """No square of 0.8 .. 1.0 of the area fits these frames: ten failed attempts (two uniform draws each, nothing else), then the
    central square."""
    from mico_amd.model.transforms import random_resized_crop_params
    H, W = size
    for seed in range(5):
        g, g_ref = _gen(seed), _gen(seed)
        assert random_resized_crop_params(H, W, generator=g) == FALLBACK[size]
        for _ in range(20):
            torch.empty(1).uniform_(0.0, 1.0, generator=g_ref)
        assert torch.equal(g.get_state(), g_ref.get_state())


@pytest.mark.parametrize("size", [(224, 224), (40, 44)])
def test_random_boxes(size):
    from mico_amd.model.transforms import random_resized_crop_params
    H, W = size
    boxes = set()
    for seed in range(40):
        g = _gen(seed)
        top, left, h, w = box = random_resized_crop_params(H, W, generator=g)
        assert box == AO.get_params(H, W, (0.8, 1.0), (1.0, 1.0), _gen(seed))
        assert h == w and 0 <= top and top + h <= H and 0 <= left and left + w <= W
        # side = round(sqrt(area)), area in [0.8 H W, H W]: the side is within 0.5 of the exact root
        assert math_sqrt(0.8 * H * W) - 0.5 <= h <= math_sqrt(H * W) + 0.5
        boxes.add(box)
    assert len(boxes) > 10     # they are random


def math_sqrt(v):
    return float(np.sqrt(np.float64(v)))


def test_center_crop_plan():
    from mico_amd.model.transforms import center_crop_plan
    p = center_crop_plan(97, 301, 32)
    assert (p.top, p.left, p.ch, p.cw) == (0, 0, 97, 301) and (p.rh, p.rw) == (32, 99) and (p.oy, p.ox) == (0, 34) and p.flip == 0
    q = center_crop_plan(301, 97, 32)
    assert (q.top, q.left, q.ch, q.cw) == (0, 0, 301, 97) and (q.rh, q.rw) == (99, 32) and (q.oy, q.ox) == (34, 0) and q.flip == 0
    s = center_crop_plan(64, 64, 32)
    assert (s.rh, s.rw, s.oy, s.ox) == (32, 32, 0, 0)


def test_frame_plan_modes_and_flip_after_box():
    from mico_amd.model.transforms import frame_plan, Plan, TABLE_COLS
    assert frame_plan(37, 53, 32, "none", True) == Plan(0, 0, 37, 53, 32, 32, 0, 0, 0)
    assert frame_plan(37, 53, 32, "none", False) == Plan(0, 0, 37, 53, 32, 32, 0, 0, 0)
    assert frame_plan(97, 301, 32, "crop_flip", False) == Plan(0, 0, 97, 301, 32, 99, 0, 34, 0)
    with pytest.raises(NotImplementedError):
        frame_plan(37, 53, 32, "color_jitter", True)
    flips = []
    for seed in range(30):
        g, g_ref = _gen(seed), _gen(seed)
        p = frame_plan(224, 200, 32, "crop_flip", True, generator=g)
        box, flip = AO.draw_train(224, 200, g_ref)       # box first, then the flip, from the same stream
        assert (p.top, p.left, p.ch, p.cw) == box and p.flip == int(flip) and (p.rh, p.rw, p.oy, p.ox) == (32, 32, 0, 0)
        assert torch.equal(g.get_state(), g_ref.get_state())
        flips.append(p.flip)
    assert 0 < sum(flips) < 30
    assert len(p.row(7, 600)) == TABLE_COLS and p.row(7, 600)[:2] == [7, 600] and p.row(7, 600)[-1] == 0


def _png(path, h, w, seed):
    from PIL import Image
    img = (np.random.RandomState(seed).rand(h, w, 3) * 255).astype(np.uint8)
    Image.fromarray(img).save(str(path))
    return img


@pytest.mark.parametrize("size", [(45, 61), (61, 45)])
@pytest.mark.parametrize("enc", ["swin", "evaclip01_giant"])
def test_host_image_processor_crop_flip(tmp_path, size, enc):
    from mico_amd.model.imageprocessor import ImageProcessor, image_stats
    H, W = size
    f = tmp_path / "a.png"
    img = _png(f, H, W, seed=H)
    mean, std = image_stats(enc)
    got = ImageProcessor(32, enc, "crop_flip", training=False, device=None)(str(f))
    assert got.shape == (1, 3, 32, 32)
    assert torch.equal(got[0], AO.eval_ref(img, 32, mean, std))
    seen = set()
    for seed in range(6):
        proc = ImageProcessor(32, enc, "crop_flip", training=True, device=None, generator=_gen(seed))
        got = proc(str(f))
        box, flip = AO.draw_train(H, W, _gen(seed))
        assert torch.equal(got[0], AO.train_ref(img, box, flip, 32, mean, std)), (seed, box, flip)
        seen.add(flip)
    assert seen == {False, True}
    assert ImageProcessor(32, enc, "crop_flip", device=None)(str(tmp_path / "missing.png")) is None
    # `none` is what it was
    assert torch.equal(ImageProcessor(32, enc, "none", device=None)(str(f))[0], AO.none_ref(img, 32, mean, std))


def test_video_processor_one_plan_per_clip(tmp_path):
    from mico_amd.model.imageprocessor import image_stats
    from mico_amd.model.videoprocessor import VideoProcessor
    d = tmp_path / "clip"
    os.makedirs(d)
    frames = [_png(d / f"img_{i + 1:04d}.png", 60, 80, seed=i) for i in range(4)]
    mean, std = image_stats("evaclip01_giant")
    for seed in range(4):
        g = _gen(seed)
        vp = VideoProcessor(32, "evaclip01_giant", sample_num=4, video_transforms="crop_flip", training=True, device=None, generator=g)
        out = vp(str(d))      # 4 frames, 4 groups of one: every frame is picked whatever random.choice does
        assert out.shape == (4, 3, 32, 32)
        g_ref = _gen(seed)
        box, flip = AO.draw_train(60, 80, g_ref)
        for k in range(4):
            assert torch.equal(out[k], AO.train_ref(frames[k], box, flip, 32, mean, std))
        assert torch.equal(g.get_state(), g_ref.get_state())     # ONE box and ONE flip were drawn for the four frames
    ev = VideoProcessor(32, "evaclip01_giant", sample_num=4, video_transforms="crop_flip", training=False, device=None)(str(d))
    for k in range(4):
        assert torch.equal(ev[k], AO.eval_ref(frames[k], 32, mean, std))
    # frames of unequal size within one clip: an error, swallowed to None
    _png(d / "img_0003.png", 61, 80, seed=9)
    for training in (True, False):
        assert VideoProcessor(32, "evaclip01_giant", sample_num=4, video_transforms="crop_flip", training=training, device=None)(str(d)) is None
    with pytest.raises(NotImplementedError):
        VideoProcessor(32, "evaclip01_giant", video_transforms="color_jitter")


def test_table_validation():
    from mico_amd.model.transforms import Plan, validate_table
    H, W, r = 20, 30, 8
    nbytes = H * W * 3
    good = Plan(2, 3, 18, 27, 8, 8, 0, 0, 1).row(0, 3 * W)
    validate_table([good], [(H, W)], nbytes, r, r)
    validate_table([Plan(0, 0, H, W, 8, 12, 0, 4, 0).row(5, 3 * W)], [(H, W)], nbytes + 5, r, r)

    def bad(row, nb=nbytes, sizes=((H, W),)):
        with pytest.raises(ValueError):
            validate_table([row], list(sizes), nb, r, r)

    bad(Plan(3, 3, 18, 27, 8, 8, 0, 0, 0).row(0, 3 * W))      # region past the bottom edge
    bad(Plan(2, 4, 18, 27, 8, 8, 0, 0, 0).row(0, 3 * W))      # region past the right edge
    bad(Plan(-1, 0, 18, 27, 8, 8, 0, 0, 0).row(0, 3 * W))
    bad(Plan(0, 0, 0, 27, 8, 8, 0, 0, 0).row(0, 3 * W))       # empty region
    bad(Plan(0, 0, H, W, 8, 12, 0, 5, 0).row(0, 3 * W))       # window past the resized image
    bad(Plan(0, 0, H, W, 7, 8, 0, 0, 0).row(0, 3 * W))        # resized image smaller than the output
    bad(Plan(0, 0, H, W, 8, 8, -1, 0, 0).row(0, 3 * W))
    bad(good, nb=nbytes - 1)                                   # frame past the end of the buffer
    bad(Plan(2, 3, 18, 27, 8, 8, 0, 0, 1).row(1, 3 * W))      # the same, by its offset
    bad(Plan(2, 3, 18, 27, 8, 8, 0, 0, 1).row(0, 3 * W - 1))  # rows that overlap
    bad(Plan(2, 3, 18, 27, 8, 8, 0, 0, 2).row(0, 3 * W))      # flip is 0 / 1
    bad(good[:-1])
    with pytest.raises(ValueError):
        validate_table([good, good], [(H, W)], nbytes, r, r)


def test_binding():
    from mico_amd import _lib
    l = _lib.lib()
    assert l.mico_version() == _lib.ABI_VERSION >= 123
    assert len(_lib.PROTOTYPES["mico_image_augment"]) == 14
    # argument checks run on the host, before any launch: no pointer is dereferenced, so host addresses will do here
    import ctypes
    buf = (ctypes.c_int64 * 12)()
    p = ctypes.addressof(buf)
    EINVAL = -22
    args = lambda src, nbytes, tab, n, dst, oh, ow: (src, nbytes, tab, n, dst, oh, ow, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None)
    for bad in (args(None, 16, p, 1, p, 8, 8), args(p, 16, None, 1, p, 8, 8), args(p, 16, p, 1, None, 8, 8), args(p, 16, p, 0, p, 8, 8),
                args(p, 16, p, -3, p, 8, 8), args(p, 16, p, 1, p, 0, 8), args(p, 16, p, 1, p, 8, -1), args(p, 0, p, 1, p, 8, 8)):
        assert l.mico_image_augment(*bad) == EINVAL
        assert b"mico_image_augment" in l.mico_last_error_string()
