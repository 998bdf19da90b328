"""Reference composition of the vision transforms for the tests of mico_amd/model/transforms.py and mico_image_augment: torch CPU operations
in torchvision's order (crop, bilinear resize without antialias, flip, Normalize; evaluation: resize the shorter side, slice the centre
window), and an independent restatement of torchvision 0.15.2's RandomResizedCrop.get_params.  Nothing here imports the code under test."""
import math

import torch
import torch.nn.functional as F


def get_params(H, W, scale, ratio, generator=None):
    """RandomResizedCrop.get_params(img, scale, ratio) -> (i, j, h, w), restated from the published source."""
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _attempt in range(10):
        frac = torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        log_r = torch.empty(1).uniform_(lo, hi, generator=generator)
        aspect_ratio = torch.exp(log_r).item()
        target_area = H * W * frac
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            i = int(torch.randint(0, H - h + 1, size=(1,), generator=generator))
            j = int(torch.randint(0, W - w + 1, size=(1,), generator=generator))
            return i, j, h, w
    in_ratio = W / H
    if in_ratio < min(ratio):
        w, h = W, int(round(W / min(ratio)))
    elif in_ratio > max(ratio):
        h, w = H, int(round(H * max(ratio)))
    else:
        h, w = H, W
    return (H - h) // 2, (W - w) // 2, h, w


def normalize(x, mean, std):
    mean = torch.tensor(mean, dtype=x.dtype).view(3, 1, 1)
    std = torch.tensor(std, dtype=x.dtype).view(3, 1, 1)
    return (x - mean) / std


def resize(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=False)


def to_float(u8):
    """uint8 [H, W, 3] (numpy or torch) -> float [1, 3, H, W] in [0, 1] (ToTensor)."""
    return torch.as_tensor(u8).permute(2, 0, 1).float().div(255.0).unsqueeze(0)


def train_ref(u8, box, flip, r, mean, std):
    """RandomResizedCrop with the given box, RandomHorizontalFlip with the given outcome, Normalize -> [3, r, r]."""
    i, j, h, w = box
    x = resize(to_float(u8)[:, :, i:i + h, j:j + w], (r, r))
    if flip:
        x = x.flip(-1)
    return normalize(x, mean, std)[0]


def eval_ref(u8, r, mean, std):
    """Resize(r) (shorter side to r, longer to int(r * long / short)), CenterCrop(r), Normalize -> [3, r, r]."""
    H, W = u8.shape[0], u8.shape[1]
    if W <= H:
        size = (int(r * H / W), r)
    else:
        size = (r, int(r * W / H))
    x = resize(to_float(u8), size)
    top, left = int(round((size[0] - r) / 2.0)), int(round((size[1] - r) / 2.0))
    return normalize(x[:, :, top:top + r, left:left + r], mean, std)[0]


def none_ref(u8, r, mean, std):
    return normalize(resize(to_float(u8), (r, r)), mean, std)[0]


def draw_train(H, W, generator):
    """the box, then the flip, as Compose([RandomResizedCrop(r, [0.8, 1.0], [1.0, 1.0]), RandomHorizontalFlip()]) draws them"""
    box = get_params(H, W, (0.8, 1.0), (1.0, 1.0), generator)
    flip = bool(torch.rand(1, generator=generator) < 0.5)
    return box, flip
