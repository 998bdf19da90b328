"""Sampling plans of the reference's vision transforms (`--vision_transforms none | crop_flip`; model/imageprocessor.py:25-40,
model/videoprocessor.py:35-50, data/data/vision_mapper.py:54-77), pure host code.

A plan says which region of a decoded frame is sampled (the crop box, or the whole frame), how large the virtual resized image of that
region is, where the resolution x resolution output window sits inside it and whether the window is mirrored:

    none                  Resize((r, r))                                   whole frame -> r x r
    crop_flip, training   RandomResizedCrop(r, [0.8, 1.0], [1.0, 1.0])     random box -> r x r, then
                          RandomHorizontalFlip()                           a flip with probability 0.5, drawn after the box
    crop_flip, evaluation Resize(r), CenterCrop(r)                         shorter side -> r, the central r x r window

One plan plus (byte offset, row pitch) is one row of mico_image_augment's table (include/mico_hip.h), which applies crop, resize, window,
flip and Normalize in one pass on the device; apply_plan_host composes the same thing from torch CPU operations.

torchvision is not available here.  random_resized_crop_params and center_crop_plan restate torchvision 0.15.2's
RandomResizedCrop.get_params, Resize (shorter-side form) and CenterCrop from their published source, in their draw order, so equal torch
seeds should give equal boxes - but parity with torchvision's random stream is UNPINNED, like the resize itself: no
test here compares against torchvision."""
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

TABLE_COLS = 12    # off, pitch, top, left, ch, cw, rh, rw, oy, ox, flip, reserved
TRANSFORMS = ("none", "crop_flip")
CROP_SCALE = (0.8, 1.0)     # the reference's RandomResizedCrop arguments
CROP_RATIO = (1.0, 1.0)


class Plan(NamedTuple):
    top: int
    left: int
    ch: int
    cw: int
    rh: int
    rw: int
    oy: int
    ox: int
    flip: int

    def row(self, off, pitch):
        """the table row of a frame that starts at byte `off` of the staging buffer with rows `pitch` bytes apart"""
        return [int(off), int(pitch), *[int(v) for v in self], 0]


def random_resized_crop_params(H, W, scale=CROP_SCALE, ratio=CROP_RATIO, generator=None):
    """torchvision 0.15.2 RandomResizedCrop.get_params -> (top, left, h, w): up to 10 attempts, each drawing the area fraction and then
    the log aspect ratio with torch.empty(1).uniform_, then (accepted attempt only) top and left with torch.randint; after 10 failures
    the central crop at the nearest legal aspect ratio."""
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            top = torch.randint(0, H - h + 1, size=(1,), generator=generator).item()
            left = torch.randint(0, W - w + 1, size=(1,), generator=generator).item()
            return top, left, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def center_crop_plan(H, W, r):
    """Resize(r) then CenterCrop(r): the shorter side goes to r, the longer one to int(r * long / short); the window offset on an axis is
    int(round((resized - r) / 2.0)) (Python's round, as torchvision's center_crop)."""
    if W <= H:
        rw, rh = r, int(r * H / W)
    else:
        rh, rw = r, int(r * W / H)
    return Plan(0, 0, H, W, rh, rw, int(round((rh - r) / 2.0)), int(round((rw - r) / 2.0)), 0)


def frame_plan(H, W, resolution, transforms, training, generator=None):
    """The plan of one frame (or of one clip: a video draws once and uses the plan for every frame)."""
    r = resolution
    if transforms == "none":
        return Plan(0, 0, H, W, r, r, 0, 0, 0)
    if transforms != "crop_flip":
        raise NotImplementedError(transforms)
    if not training:
        return center_crop_plan(H, W, r)
    top, left, h, w = random_resized_crop_params(H, W, generator=generator)
    flip = int(bool(torch.rand(1, generator=generator) < 0.5))     # RandomHorizontalFlip(p=0.5), after the box
    return Plan(top, left, h, w, r, r, 0, 0, flip)


def validate_table(rows, frame_sizes, src_bytes, out_h, out_w):
    """Host check of a table before any launch: every frame lies inside the staging buffer, every region inside its frame, every output
    window inside its virtual resized image.  rows: n rows of TABLE_COLS integers; frame_sizes: n (H, W).  Raises ValueError."""
    if len(rows) != len(frame_sizes) or not rows:
        raise ValueError(f"table has {len(rows)} rows for {len(frame_sizes)} frames")
    for i, (row, (H, W)) in enumerate(zip(rows, frame_sizes)):
        if len(row) != TABLE_COLS:
            raise ValueError(f"row {i}: {len(row)} columns, expected {TABLE_COLS}")
        off, pitch, top, left, ch, cw, rh, rw, oy, ox, flip, reserved = [int(v) for v in row]
        if H < 1 or W < 1 or off < 0 or pitch < 3 * W or off + (H - 1) * pitch + 3 * W > src_bytes:
            raise ValueError(f"row {i}: frame {H}x{W} at byte {off} (pitch {pitch}) does not lie inside the {src_bytes}-byte buffer")
        if top < 0 or left < 0 or ch < 1 or cw < 1 or top + ch > H or left + cw > W:
            raise ValueError(f"row {i}: region (top {top}, left {left}, {ch}x{cw}) does not lie inside the {H}x{W} frame")
        if rh < 1 or rw < 1 or oy < 0 or ox < 0 or oy + out_h > rh or ox + out_w > rw:
            raise ValueError(f"row {i}: window {out_h}x{out_w} at ({oy}, {ox}) does not lie inside the {rh}x{rw} resized image")
        if flip not in (0, 1) or reserved != 0:
            raise ValueError(f"row {i}: flip must be 0 or 1 and the reserved column 0")


def apply_plan_host(img, plan, resolution, mean, std):
    """img: float [..., 3, H, W] in [0, 1] -> [..., 3, r, r]: crop, bilinear resize (no antialias), window, flip, Normalize with torch
    CPU operations - what mico_image_augment computes in one pass."""
    r = resolution
    lead = img.shape[:-3]
    x = img.reshape(-1, *img.shape[-3:])
    x = x[:, :, plan.top:plan.top + plan.ch, plan.left:plan.left + plan.cw]
    x = F.interpolate(x, size=(plan.rh, plan.rw), mode="bilinear", align_corners=False, antialias=False)
    x = x[:, :, plan.oy:plan.oy + r, plan.ox:plan.ox + r]
    if plan.flip:
        x = x.flip(-1)
    mean = torch.tensor(mean, dtype=x.dtype).view(3, 1, 1)
    std = torch.tensor(std, dtype=x.dtype).view(3, 1, 1)
    return ((x - mean) / std).reshape(*lead, 3, r, r)


def pack_frames(frames, pin=False):
    """frames: uint8 numpy / torch arrays [H, W, 3] of any sizes -> (one uint8 staging buffer with the frames back to back, byte offsets).
    pin=True allocates the buffer in pinned host memory, so its host-to-device copy is one asynchronous transfer."""
    sizes = [int(f.shape[0]) * int(f.shape[1]) * 3 for f in frames]
    offs = [0]
    for s in sizes[:-1]:
        offs.append(offs[-1] + s)
    buf = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=pin)
    for f, o, s in zip(frames, offs, sizes):
        assert f.ndim == 3 and f.shape[2] == 3
        buf[o:o + s] = torch.as_tensor(f, dtype=torch.uint8).reshape(-1)
    return buf, offs
