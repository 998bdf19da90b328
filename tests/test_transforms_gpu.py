"""mico_image_augment (batched crop / resize / flip / normalise) and the processors built on it, against the torch CPU composition of
tests/augment_oracle.py.  Every comparison is held to the bound of test_processors_gpu.py::test_image_and_frames: 2e-6 * max(1, max |ref|)."""
import os
import re

import numpy as np
import pytest
import torch

import augment_oracle as AO

pytestmark = pytest.mark.gpu

MEAN, STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]


def _img(h, w, seed):
    return (np.random.RandomState(seed).rand(h, w, 3) * 255).astype(np.uint8)


def _close(got, ref, what=None):
    err = (got.cpu() - ref).abs().max().item()
    bound = 2e-6 * max(1.0, ref.abs().max().item())
    assert err < bound, (what, err, bound)


def _run(cuda, frames, plans, r):
    from mico_amd.model.videoprocessor import augment_frames_device
    out = augment_frames_device(frames, plans, r, MEAN, STD, cuda)
    assert out.shape == (len(frames), 3, r, r) and out.dtype == torch.float32 and out.is_cuda
    return out


@pytest.mark.parametrize("r", [32, 30])     # 30: rows that are no multiple of four pixels (4-byte stores, a ragged last run)
def test_kernel_against_oracle_injected_plans(cuda, r):
    from mico_amd.model.transforms import Plan, center_crop_plan
    frames, plans, refs, names = [], [], [], []
    for k, (h, w) in enumerate(((37, 53), (53, 37), (20, 31))):      # 20 x 31: upsampling
        img = _img(h, w, k)
        boxes = [(0, 0, h, w), (3, 5, h - 7, w - 9), (h - 17, w - 19, 17, 19), (1, 0, 9, 30 if w > 30 else w - 1)]
        for box in boxes:
            for flip in (0, 1):
                frames.append(img)
                plans.append(Plan(*box, r, r, 0, 0, flip))
                refs.append(AO.train_ref(img, box, flip, r, MEAN, STD))
                names.append((h, w, box, flip))
    for k, (h, w) in enumerate(((97, 301), (301, 97), (64, 64))):    # the evaluation plan: shorter side to r, centre window
        img = _img(h, w, 10 + k)
        frames.append(img)
        plans.append(center_crop_plan(h, w, r))
        refs.append(AO.eval_ref(img, r, MEAN, STD))
        names.append((h, w, "eval"))
        frames.append(img)
        plans.append(Plan(0, 0, h, w, r, r, 0, 0, 0))                # `none`
        refs.append(AO.none_ref(img, r, MEAN, STD))
        names.append((h, w, "none"))
    out = _run(cuda, frames, plans, r)
    for o, ref, name in zip(out, refs, names):
        _close(o, ref, name)


def test_identity_scale_224(cuda):
    """224 x 224 at resolution 224: the identity resize (every weight 0 or 1) with and without flip, and a crop of it that upsamples."""
    from mico_amd.model.transforms import Plan
    img = _img(224, 224, 5)
    plans = [Plan(0, 0, 224, 224, 224, 224, 0, 0, 0), Plan(0, 0, 224, 224, 224, 224, 0, 0, 1), Plan(11, 7, 200, 200, 224, 224, 0, 0, 1)]
    out = _run(cuda, [img] * 3, plans, 224)
    _close(out[0], AO.none_ref(img, 224, MEAN, STD), "identity")
    ident = AO.normalize(AO.to_float(img), MEAN, STD)[0]
    _close(out[0], ident, "identity pixels")
    _close(out[1], ident.flip(-1), "identity flipped")
    _close(out[2], AO.train_ref(img, (11, 7, 200, 200), True, 224, MEAN, STD), "crop 200")


@pytest.mark.parametrize("r", [32, 30])
def test_neighbours_clamp_at_the_region_edge(cuda, r):
    """A box of zeros that touches nothing but 255s: its right and bottom neighbours inside the frame are 255, and so are the frame's last
    column / row when the box ends there.  Any tap outside the box would lift a sample above the normalised zero."""
    from mico_amd.model.transforms import Plan
    frames, plans = [], []
    for (h, w, box) in ((40, 50, (5, 6, 21, 23)), (40, 50, (19, 27, 21, 23)), (24, 26, (0, 0, 23, 25)), (33, 21, (0, 0, 33, 20)),
                        (21, 33, (0, 0, 20, 33))):
        img = np.full((h, w, 3), 255, dtype=np.uint8)
        t, l, bh, bw = box
        img[t:t + bh, l:l + bw] = 0
        for flip in (0, 1):
            frames.append(img)
            plans.append(Plan(t, l, bh, bw, r, r, 0, 0, flip))
    out = _run(cuda, frames, plans, r).cpu()
    zero = (np.float32(0.0) - np.array(MEAN, dtype=np.float32)) * np.array([1.0 / s for s in STD], dtype=np.float32)   # the kernel's own arithmetic
    want = torch.from_numpy(zero).view(1, 3, 1, 1).expand_as(out)
    assert torch.equal(out, want)
    _close(out[0], AO.normalize(torch.zeros(1, 3, r, r), MEAN, STD)[0], "normalised zero")


def test_ragged_batch_equals_one_row_launches(cuda):
    """Seven frames with odd byte counts, so every offset but the first is unaligned and of every residue mod 4; the last frame ends the
    buffer, so its last taps take the clamped byte loads.  A frame's bits do not depend on its slot or on its neighbours."""
    from mico_amd.model.transforms import Plan, frame_plan, pack_frames
    sizes = [(37, 53), (21, 33), (53, 37), (15, 17), (41, 29), (33, 35), (27, 31)]
    assert all((h * w * 3) % 2 == 1 for h, w in sizes)
    frames = [_img(h, w, 20 + k) for k, (h, w) in enumerate(sizes)]
    _, offs = pack_frames(frames)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    g = torch.Generator().manual_seed(3)
    for r in (32, 30):
        plans = [frame_plan(h, w, r, "crop_flip", k % 3 != 0, generator=g) if k != 6 else Plan(0, 0, 27, 31, r, r, 0, 0, k % 2)
                 for k, (h, w) in enumerate(sizes)]
        assert plans[6].top + plans[6].ch == 27 and plans[6].left + plans[6].cw == 31       # reads the last byte of the buffer
        out = _run(cuda, frames, plans, r)
        for k, (f, p) in enumerate(zip(frames, plans)):
            one = _run(cuda, [f], [p], r)
            assert torch.equal(out[k], one[0]), (r, k)
            if p.rh == p.rw == r:
                ref = AO.train_ref(f, (p.top, p.left, p.ch, p.cw), p.flip, r, MEAN, STD)
            else:
                ref = AO.eval_ref(f, r, MEAN, STD)
            _close(out[k], ref, (r, k))


def test_entry_rejects_bad_arguments_and_tables(cuda):
    from mico_amd import _lib
    from mico_amd.model.transforms import Plan
    from mico_amd.model.videoprocessor import augment_packed_device
    img = torch.from_numpy(_img(20, 30, 1))
    with pytest.raises(ValueError):       # the host validation stops a region outside its frame before any launch
        augment_packed_device(img.reshape(-1), [Plan(0, 0, 21, 30, 8, 8, 0, 0, 0).row(0, 90)], [(20, 30)], 8, MEAN, STD, cuda)
    src = img.reshape(-1).to(cuda)
    tab = torch.tensor([Plan(0, 0, 20, 30, 8, 8, 0, 0, 0).row(0, 90)], dtype=torch.int64, device=cuda)
    out = torch.empty(1, 3, 8, 8, device=cuda)
    l = _lib.lib()
    tail = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None)
    assert l.mico_image_augment(src.data_ptr(), src.numel(), tab.data_ptr(), 0, out.data_ptr(), 8, 8, *tail) == -22
    assert l.mico_image_augment(src.data_ptr(), src.numel(), tab.data_ptr(), 1, out.data_ptr(), 0, 8, *tail) == -22
    assert l.mico_image_augment(src.data_ptr(), src.numel(), None, 1, out.data_ptr(), 8, 8, *tail) == -22


def _files(tmp_path, sizes):
    from PIL import Image
    files = []
    for k, (h, w) in enumerate(sizes):
        f = str(tmp_path / f"i{k}_{h}_{w}.png")
        Image.fromarray(_img(h, w, 40 + k)).save(f)
        files.append(f)
    return files


def test_device_processors_against_host(cuda, tmp_path):
    from mico_amd.model.imageprocessor import ImageProcessor
    from mico_amd.model.videoprocessor import VideoProcessor
    files = _files(tmp_path, [(45, 61), (61, 45)])
    for enc in ("swin", "evaclip01_giant"):
        for training in (True, False):
            for f in files:
                host = ImageProcessor(32, enc, "crop_flip", training=training, generator=torch.Generator().manual_seed(11))(f)
                dev = ImageProcessor(32, enc, "crop_flip", training=training, device=cuda, generator=torch.Generator().manual_seed(11))(f)
                assert dev.is_cuda and dev.shape == (1, 3, 32, 32)
                _close(dev, host, (enc, training, f))
    d = tmp_path / "clip"
    os.makedirs(d)
    from PIL import Image
    for i in range(4):
        Image.fromarray(_img(60, 80, 60 + i)).save(str(d / f"img_{i + 1:04d}.png"))
    for training in (True, False):
        kw = dict(sample_num=4, video_transforms="crop_flip", training=training)
        host = VideoProcessor(32, "evaclip01_giant", device=None, generator=torch.Generator().manual_seed(5), **kw)(str(d))
        dev = VideoProcessor(32, "evaclip01_giant", device=cuda, generator=torch.Generator().manual_seed(5), **kw)(str(d))
        assert dev.shape == (4, 3, 32, 32)
        _close(dev, host, ("video", training))


def test_image_batch(cuda, tmp_path):
    from mico_amd.model.imageprocessor import ImageProcessor
    files = _files(tmp_path, [(45, 61), (61, 45), (33, 35), (70, 41)])
    files.insert(2, str(tmp_path / "missing.png"))
    for transforms, training in (("crop_flip", True), ("crop_flip", False), ("none", False)):
        proc = ImageProcessor(32, "evaclip01_giant", transforms, training=training, device=cuda, generator=torch.Generator().manual_seed(9))
        pixels, kept = proc.batch(files)
        assert kept == [0, 1, 3, 4] and pixels.shape == (4, 1, 3, 32, 32) and pixels.is_cuda
        single = ImageProcessor(32, "evaclip01_giant", transforms, training=training, device=cuda, generator=torch.Generator().manual_seed(9))
        host = ImageProcessor(32, "evaclip01_giant", transforms, training=training, generator=torch.Generator().manual_seed(9))
        for k, i in enumerate(kept):       # the same draws in the same order: the missing file draws nothing
            one = single(files[i])
            if transforms == "crop_flip":  # the same kernel: the same bits (`none` single-file calls keep mico_image_preprocess)
                assert torch.equal(pixels[k], one)
            _close(pixels[k], one.cpu(), (transforms, training, i))
            _close(pixels[k], host(files[i]), (transforms, training, i, "host"))
        assert single(files[2]) is None
    pixels, kept = proc.batch([files[2]])
    assert kept == [] and pixels.shape == (0, 1, 3, 32, 32)


def test_video_batch(cuda, tmp_path):
    from PIL import Image
    from mico_amd.model.videoprocessor import VideoProcessor
    folders, clips = [], []
    for c, (h, w) in enumerate(((60, 80), (45, 33), (52, 52))):     # clips differ in size; frames within a clip do not
        d = tmp_path / f"clip{c}"
        os.makedirs(d)
        frames = [_img(h, w, 100 + 10 * c + i) for i in range(3)]
        for i, a in enumerate(frames):
            Image.fromarray(a).save(str(d / f"img_{i + 1:04d}.png"))
        folders.append(str(d))
        clips.append(frames)
    folders.insert(1, str(tmp_path / "missing"))
    bad = tmp_path / "ragged"                                        # unequal frames within one clip: skipped, like a missing folder
    os.makedirs(bad)
    for i, (h, w) in enumerate(((20, 20), (20, 21), (20, 20))):
        Image.fromarray(_img(h, w, i)).save(str(bad / f"img_{i + 1:04d}.png"))
    folders.append(str(bad))
    g = torch.Generator().manual_seed(21)
    vp = VideoProcessor(32, "evaclip01_giant", sample_num=3, video_transforms="crop_flip", training=True, device=cuda, generator=g)
    pixels, kept = vp.batch(folders)
    assert kept == [0, 2, 3] and pixels.shape == (3, 3, 3, 32, 32) and pixels.is_cuda
    g_ref = torch.Generator().manual_seed(21)
    for k, frames in enumerate(clips):
        box, flip = AO.draw_train(frames[0].shape[0], frames[0].shape[1], g_ref)     # one plan per clip, clips in order
        for i, a in enumerate(frames):
            _close(pixels[k, i], AO.train_ref(a, box, flip, 32, MEAN, STD), (k, i))
    assert torch.equal(g.get_state(), g_ref.get_state())
    ev, kept = VideoProcessor(32, "evaclip01_giant", sample_num=3, video_transforms="crop_flip", training=False, device=cuda).batch(folders)
    assert kept == [0, 2, 3]
    for k, frames in enumerate(clips):
        for i, a in enumerate(frames):
            _close(ev[k, i], AO.eval_ref(a, 32, MEAN, STD), (k, i, "eval"))


def test_demo_transforms(cuda, tmp_path, capsys):
    """inference_demo.py --transforms crop_flip (evaluation: shorter side + centre window) changes the lines of a non-square image and
    feeds --video's frames through the video processor: one more finite [1, len(texts)] similarity.  (2-block tower, as
    tests/test_audio_frontend_gpu.py.)"""
    import inference_demo as demo
    from mico_amd import runtime
    from PIL import Image
    img = str(tmp_path / "test.png")
    Image.fromarray(_img(150, 300, 0)).save(img)
    d = tmp_path / "clip"
    os.makedirs(d)
    for i in range(5):
        Image.fromarray(_img(120, 200, 200 + i)).save(str(d / f"img_{i + 1:04d}.png"))
    pdir = str(tmp_path / "MiCo-synth")
    demo.write_synthetic_pretrain_dir(pdir, "evaclip02_base", steps=(3, 12), vision_layers=2, max_vision_sample_num=4)
    texts = ["a man is skiing in a snowy day.", "two dogs"]
    old = runtime.compute_dtype()
    try:
        capsys.readouterr()
        demo.main(["--pretrain_dir", pdir, "--image", img, "--texts", *texts])
        base = capsys.readouterr().out
        demo.main(["--pretrain_dir", pdir, "--image", img, "--texts", *texts, "--transforms", "crop_flip", "--video", str(d)])
        crop = capsys.readouterr().out
    finally:
        runtime.set_compute_dtype(old)
    base, crop = base.strip().splitlines(), crop.strip().splitlines()
    assert len(base) >= 4 and len(crop) == len(base) + 1
    assert crop[:-1] != base                       # the centre window is another picture than the squashed frame
    extra = crop[-1]
    sim = [float(v) for v in re.findall(r"-?\d+\.\d*(?:e[-+]?\d+)?", extra)]
    assert extra.startswith("tensor([[") and len(sim) == len(texts) and all(abs(v) <= 1.0 + 1e-3 for v in sim), extra
