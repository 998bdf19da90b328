"""Host-side image preprocessing with the reference's surface (model/imageprocessor.py:10-63): PIL decode -> RGB -> [0,1] CHW
float tensor -> Resize((r, r)) -> Normalize(mean, std) -> (1, 3, r, r).  Mean/std are chosen by the encoder-type string exactly
as the reference does (CLIP statistics for 'clip*'/'evaclip*', ImageNet otherwise - note inference_demo.py passes "swin").
torchvision is not available here: Resize is restated as bilinear interpolation without antialiasing, which is what
torchvision 0.15's Resize does for tensor inputs (resize parity itself is unpinned).  Decoding/resizing is
host I/O outside the hot path; the tensor it emits is where the MI355X path starts.
image_transforms="crop_flip" (RandomResizedCrop + RandomHorizontalFlip in training, Resize + CenterCrop in evaluation) draws a sampling
plan on the host (transforms.frame_plan) and applies it either with torch CPU operations (device=None) or in one mico_image_augment
launch; batch() sends a whole list of files, ragged in size, through one copy and one launch."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import transforms as T


def image_stats(encoder_type):
    """imageprocessor.py:17-22 / videoprocessor.py:27-33: CLIP statistics for clip* / evaclip*, ImageNet otherwise."""
    if encoder_type.startswith("clip") or encoder_type.startswith("evaclip"):
        return [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]
    return [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


class ImageProcessor(object):
    def __init__(self, image_resolution, image_encoder_type, image_transforms="none", training=True, device=None, generator=None):
        """device=None: host path (torch ops); device="cuda": decode on the host, then ToTensor + Resize + Normalize in one
        device kernel (mico_image_preprocess; mico_image_augment for crop_flip and batch()) - the returned tensor already lives on the
        device.  generator: the torch.Generator of the crop_flip draws (None: torch's global one)."""
        self.training = training
        self.resolution = image_resolution
        self.image_encoder_type = image_encoder_type
        self.device = device
        self.mean, self.std = image_stats(image_encoder_type)
        if image_transforms not in T.TRANSFORMS:
            raise NotImplementedError(image_transforms)
        self.image_transforms = image_transforms
        self.generator = generator

    def transform(self, img):
        """img: float CHW tensor in [0,1] -> resized + normalised CHW."""
        r = self.resolution
        img = F.interpolate(img.unsqueeze(0), size=(r, r), mode="bilinear", align_corners=False, antialias=False)[0]
        mean = torch.tensor(self.mean, dtype=img.dtype).view(3, 1, 1)
        std = torch.tensor(self.std, dtype=img.dtype).view(3, 1, 1)
        return (img - mean) / std

    def _decode(self, image_file):
        """-> uint8 [H, W, 3] tensor, or None for a missing file."""
        if not os.path.exists(image_file):
            print("not have image", image_file)
            return None
        from PIL import Image
        img = Image.open(image_file).convert("RGB")
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())

    def _plan(self, u8):
        return T.frame_plan(u8.shape[0], u8.shape[1], self.resolution, self.image_transforms, self.training, self.generator)

    def __call__(self, image_file):
        try:
            u8 = self._decode(image_file)
            if u8 is None:
                return None
            if self.image_transforms == "none":
                if self.device is not None:
                    from .videoprocessor import preprocess_frames_device
                    return preprocess_frames_device(u8.unsqueeze(0), self.resolution, self.mean, self.std, self.device)
                return self.transform(u8.permute(2, 0, 1).float().div(255.0)).unsqueeze(0)
            plan = self._plan(u8)
            if self.device is not None:
                from .videoprocessor import augment_frames_device
                return augment_frames_device([u8], [plan], self.resolution, self.mean, self.std, self.device)
            return T.apply_plan_host(u8.permute(2, 0, 1).float().div(255.0), plan, self.resolution, self.mean, self.std).unsqueeze(0)
        except Exception as e:   # the reference swallows errors and returns None (imageprocessor.py:61-63)
            print(e)
            return None

    def batch(self, image_files):
        """-> (pixels [k, 1, 3, r, r] on the device, kept): every file that decoded, in order; kept lists their indices in image_files
        (the others are reported and skipped, as __call__ returns None for them).  The decoded images, ragged in size, take one
        host-to-device copy and one mico_image_augment launch; image_transforms="none" goes the same way."""
        if self.device is None:
            raise ValueError("ImageProcessor.batch runs on the device: construct the processor with device='cuda'")
        frames, plans, kept = [], [], []
        for i, f in enumerate(image_files):
            try:
                u8 = self._decode(f)
                if u8 is None:
                    continue
                plan = self._plan(u8)
            except Exception as e:
                print(e)
                continue
            frames.append(u8)
            plans.append(plan)
            kept.append(i)
        r = self.resolution
        if not kept:
            return torch.empty((0, 1, 3, r, r), dtype=torch.float32, device=self.device), kept
        from .videoprocessor import augment_frames_device
        return augment_frames_device(frames, plans, r, self.mean, self.std, self.device).unsqueeze(1), kept
