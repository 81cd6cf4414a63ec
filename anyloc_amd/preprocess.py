"""Device-side ingest: uint8 HWC images -> ImageNet-normalised float CHW
batches cropped to multiples of the patch size, in one HIP kernel -- the work the reference does per
image on the host with ``ToTensor() + Normalize`` (``dvgl_benchmark/datasets_ws.py:20-23``) and
``CenterCrop((h//14*14, w//14*14))`` (``scripts/dino_v2_vlad.py:173-176``) before every extractor call.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .synth import IMAGENET_MEAN, IMAGENET_STD, PATCH


def _centre(full, part):
    return int(round((full - part) / 2.0))          # torchvision CenterCrop: round half to even


def resize_bicubic(x, size, crop=None, out=None):
    """x float [B,3,H,W] (device) -> bicubic resize to ``size=(h,w)`` (torch's kernel, align_corners=False, no
    antialias = ``T.resize(img, (h, w), BICUBIC)`` of a tensor in the torchvision the reference pins), optionally
    centre-cropped to ``crop=(ch,cw)`` in the same kernel; ``out``: the contiguous float32 device tensor to write into."""
    dev = _lib.require_gpu()
    x = x.to(dev, torch.float32).contiguous()
    B, Cn, H, W = x.shape
    h, w = int(size[0]), int(size[1])
    ch, cw = (h, w) if crop is None else (int(crop[0]), int(crop[1]))
    if out is None:
        out = torch.empty(B, Cn, ch, cw, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, Cn, ch, cw) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"resize_bicubic: out must be a contiguous float32 [{B}, {Cn}, {ch}, {cw}] tensor on {dev}")
    _lib.check(_lib.load().anyloc_resize_bicubic(_lib.ptr(x), B * Cn, H, W, h, w, _centre(h, ch), _centre(w, cw), ch, cw,
                                                 _lib.ptr(out), _lib.stream_ptr()), "anyloc_resize_bicubic")
    return out


def demo_size(h, w, max_img_size=None, multiple=PATCH):
    """(resized, cropped) sizes the demo gives an h x w image (reference demo/anyloc_vlad_generate.py:163-181): the longer
    side capped at ``max_img_size`` (aspect kept, ``int()`` truncation), then centre-cropped to multiples of ``multiple``.
    resized is None when no resize happens."""
    rs = None
    if max_img_size is not None and max(h, w) > max_img_size:
        if h == max(h, w):
            rs = (int(max_img_size), int(w * max_img_size / h))
        else:
            rs = (int(h * max_img_size / w), int(max_img_size))
        h, w = rs
    return rs, (h // multiple * multiple, w // multiple * multiple)


def images_to_input_ragged(images, max_img_size=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, multiple=PATCH):
    """Images of DIFFERENT sizes (a sequence of uint8 [H_i, W_i, 3] NumPy arrays / torch tensors) -> (flat float32 GPU
    buffer holding the [3, h_i, w_i] inputs back to back, [(h_i, w_i), ...]): every image gets what ``images_to_input``
    gives it alone (normalise, the demo's bicubic downscale above ``max_img_size``, centre crop to multiples of 14), written
    into its slice of one buffer -- the input ``HipDinoV2.forward_taps_ragged`` takes."""
    dev = _lib.require_gpu()
    plans = []
    for im in images:
        if im.ndim != 3 or im.shape[-1] != 3:
            raise ValueError(f"expected uint8 [H,W,3] images, got {tuple(im.shape)}")
        rs, crop = demo_size(int(im.shape[0]), int(im.shape[1]), max_img_size, multiple)
        if crop[0] < multiple or crop[1] < multiple:
            raise ValueError(f"image {tuple(im.shape[:2])} is smaller than one {multiple} x {multiple} patch")
        plans.append((rs, crop))
    sizes = [c for _, c in plans]
    total = sum(3 * h * w for h, w in sizes)
    flat = torch.empty(total, dtype=torch.float32, device=dev)
    at = 0
    for im, (h, w) in zip(images, sizes):
        images_to_input(im, mean, std, multiple, max_img_size=max_img_size, out=flat[at:at + 3 * h * w].view(1, 3, h, w))
        at += 3 * h * w
    return flat, sizes


def images_to_input(images, mean=IMAGENET_MEAN, std=IMAGENET_STD, multiple=PATCH, crop=None, max_img_size=None, out=None):
    """images: uint8 [B,H,W,3] (or [H,W,3]) torch tensor / numpy array, host or device.
    Returns float32 [B,3,H',W'] on the GPU with H' = H//multiple*multiple (or ``crop=(h,w)``).

    ``max_img_size`` (reference demo/anyloc_vlad_generate.py:163-181): when the longer side exceeds it, the normalised
    image is first resized (aspect kept, ``int()`` truncation as the demo computes it) with bicubic interpolation, then
    centre-cropped to multiples of ``multiple`` -- normalise, resize and crop all on the device.  ``out``: a contiguous
    float32 device tensor of the result's shape to write into."""
    dev = _lib.require_gpu()
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(np.ascontiguousarray(images))
    if images.ndim == 3:
        images = images[None]
    if images.dtype != torch.uint8 or images.shape[-1] != 3:
        raise ValueError(f"expected uint8 [B,H,W,3], got {images.dtype} {tuple(images.shape)}")
    images = images.to(dev, non_blocking=True).contiguous()
    B, H, W, _ = images.shape
    rs, cropped = demo_size(H, W, max_img_size, multiple)
    if rs is not None:
        full = images_to_input(images, mean, std, multiple, crop=(H, W))          # ToTensor + Normalize, no crop
        return resize_bicubic(full, rs, crop if crop is not None else cropped, out=out)
    ch, cw = crop if crop is not None else (H // multiple * multiple, W // multiple * multiple)
    if out is None:
        out = torch.empty(B, 3, ch, cw, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, 3, ch, cw) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"images_to_input: out must be a contiguous float32 [{B}, 3, {ch}, {cw}] tensor on {dev}")
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(_lib.load().anyloc_preprocess_u8(C.c_void_p(images.data_ptr()), B, H, W, ch, cw, m, s,
                                                _lib.ptr(out), _lib.stream_ptr()), "anyloc_preprocess_u8")
    return out
