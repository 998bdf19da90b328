"""Video / frame-folder preprocessing with the reference's surface (model/videoprocessor.py:11-108): `split` the frame list into
sample_num contiguous groups (padding with the last frame), pick one frame per group (random in training, the middle one in
evaluation), decode (PIL, host), then ToTensor + Resize + Normalize ON THE DEVICE in one kernel (mico_image_preprocess).  The
'raw' container format needs decord, which this image does not have; frame folders ('frame') are supported.
video_transforms="crop_flip" and batch() go through mico_image_augment: one plan per clip (transforms.frame_plan; the reference
transforms the stacked [n, 3, H, W] tensor, so every frame of a clip gets the same box and flip), one launch for all frames."""
import os
import random

import numpy as np
import torch

from .. import _lib
from . import transforms as T
from .imageprocessor import image_stats


def split(frame_name_lists, sample_num):
    """videoprocessor.py:11-15 / audioprocessor.py:8-12: sample_num contiguous groups whose sizes differ by at most one (the
    first len % sample_num groups get the extra element); a short list is first padded with its last element."""
    items = list(frame_name_lists)
    while len(items) < sample_num:
        items.append(items[-1])
    base, extra = divmod(len(items), sample_num)
    groups, start = [], 0
    for g in range(sample_num):
        size = base + (1 if g < extra else 0)
        groups.append(items[start:start + size])
        start += size
    return groups


def sample_indices(groups, training):
    """one element per group: random.choice in training, the (upper-)middle element otherwise (videoprocessor.py:66-69)."""
    if training:
        return [random.choice(i) for i in groups]
    return [i[(len(i) + 1) // 2 - 1] for i in groups]


def preprocess_frames_device(frames_u8, resolution, mean, std, device="cuda"):
    """uint8 [n, H, W, 3] (host or device) -> normalised fp32 [n, 3, r, r] on the device; see mico_image_preprocess."""
    x = frames_u8.to(device).contiguous()
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3
    n, H, W, _ = x.shape
    out = torch.empty((n, 3, resolution, resolution), dtype=torch.float32, device=x.device)
    rc = _lib.lib().mico_image_preprocess(x.data_ptr(), n, H, W, out.data_ptr(), resolution, resolution, mean[0], mean[1], mean[2],
                                          1.0 / std[0], 1.0 / std[1], 1.0 / std[2], torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, "mico_image_preprocess")
    return out


def augment_frames_device(frames, plans, resolution, mean, std, device="cuda"):
    """frames: decoded uint8 [H, W, 3] arrays of ANY sizes; plans: one transforms.Plan per frame -> normalised fp32 [n, 3, r, r] on the
    device.  The frames are packed back to back into one pinned staging buffer: one host-to-device copy, one table copy and one
    mico_image_augment launch for the whole ragged batch.  The table is validated on the host first."""
    buf, offs = T.pack_frames(frames, pin=True)
    sizes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
    rows = [p.row(o, 3 * w) for p, o, (_, w) in zip(plans, offs, sizes)]
    return augment_packed_device(buf, rows, sizes, resolution, mean, std, device)


def augment_packed_device(buf, rows, sizes, resolution, mean, std, device="cuda"):
    """buf: the uint8 staging buffer (host or device); rows: n table rows (transforms.Plan.row); sizes: n (H, W); see mico_image_augment."""
    T.validate_table(rows, sizes, buf.numel(), resolution, resolution)
    table = torch.tensor(rows, dtype=torch.int64)
    if buf.device.type == "cpu" and buf.is_pinned():
        table = table.pin_memory()
    src = buf.to(device, non_blocking=True)
    tab = table.to(device, non_blocking=True)
    assert src.dtype == torch.uint8 and src.is_contiguous()
    n = len(rows)
    out = torch.empty((n, 3, resolution, resolution), dtype=torch.float32, device=src.device)
    rc = _lib.lib().mico_image_augment(src.data_ptr(), src.numel(), tab.data_ptr(), n, out.data_ptr(), resolution, resolution, mean[0],
                                       mean[1], mean[2], 1.0 / std[0], 1.0 / std[1], 1.0 / std[2],
                                       torch.cuda.current_stream(src.device).cuda_stream)
    _lib.check(rc, "mico_image_augment")
    return out


class VideoProcessor(object):
    def __init__(self, video_resolution, video_encoder_type, sample_num=4, video_transforms="none", data_format="frame", training=True,
                 device="cuda", generator=None):
        self.frame_syncaug = True
        self.training = training
        self.sample_num = sample_num
        self.data_format = data_format
        self.resolution = video_resolution
        self.video_encoder_type = video_encoder_type
        self.mean, self.std = image_stats(video_encoder_type)
        self.device = device
        if video_transforms not in T.TRANSFORMS:
            raise NotImplementedError(video_transforms)
        self.video_transforms = video_transforms
        self.generator = generator     # torch.Generator of the crop_flip draws (None: torch's global one)

    def _decode(self, video_file):
        """-> the sample_num picked frames, uint8 [H, W, 3] each, or None for a missing folder."""
        if self.data_format != "frame":
            raise NotImplementedError("data_format='raw' decodes with decord, which is not available; extract frames to a folder")
        if not os.path.exists(video_file):
            print("not have videos", video_file)
            return None
        from PIL import Image
        frames = sorted(os.listdir(video_file))
        picked = sample_indices(split(frames, self.sample_num), self.training)
        return [np.array(Image.open(os.path.join(video_file, f)).convert("RGB"), dtype=np.uint8) for f in picked]

    def clip_plan(self, imgs):
        """ONE plan for the whole clip (frame_syncaug): the frames must share a size."""
        sizes = {(i.shape[0], i.shape[1]) for i in imgs}
        if len(sizes) != 1:
            raise ValueError(f"frames of one clip differ in size: {sorted(sizes)}")
        (H, W), = sizes
        return T.frame_plan(H, W, self.resolution, self.video_transforms, self.training, self.generator)

    def __call__(self, video_file):
        try:
            imgs = self._decode(video_file)
            if imgs is None:
                return None
            if self.video_transforms == "none" and self.device is not None:
                batch = torch.from_numpy(np.stack(imgs, 0))
                return preprocess_frames_device(batch, self.resolution, self.mean, self.std, self.device)
            plan = self.clip_plan(imgs)
            if self.device is None:      # host path: the reference's transforms on the stacked [n, 3, H, W] tensor
                x = torch.from_numpy(np.stack(imgs, 0)).permute(0, 3, 1, 2).float().div(255.0)
                return T.apply_plan_host(x, plan, self.resolution, self.mean, self.std)
            return augment_frames_device(imgs, [plan] * len(imgs), self.resolution, self.mean, self.std, self.device)
        except Exception as e:   # the reference swallows errors and returns None (videoprocessor.py:104-107)
            print(e)
            print(video_file)
            return None

    def batch(self, folders):
        """-> (pixels [k, sample_num, 3, r, r] on the device, kept): every folder that decoded, in order; kept lists their indices in
        `folders` (the others are reported and skipped, as __call__ returns None for them).  All frames of all clips, ragged in size
        across clips, take one host-to-device copy and one mico_image_augment launch; video_transforms="none" goes the same way."""
        if self.device is None:
            raise ValueError("VideoProcessor.batch runs on the device: construct the processor with device='cuda'")
        frames, plans, kept = [], [], []
        for i, folder in enumerate(folders):
            try:
                imgs = self._decode(folder)
                if imgs is None:
                    continue
                plan = self.clip_plan(imgs)
            except Exception as e:
                print(e)
                print(folder)
                continue
            frames += imgs
            plans += [plan] * len(imgs)
            kept.append(i)
        r = self.resolution
        if not kept:
            return torch.empty((0, self.sample_num, 3, r, r), dtype=torch.float32, device=self.device), kept
        out = augment_frames_device(frames, plans, r, self.mean, self.std, self.device)
        return out.view(len(kept), self.sample_num, 3, r, r), kept
