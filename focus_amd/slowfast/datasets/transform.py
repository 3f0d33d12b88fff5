"""Spatial sampling of a clip together with its object boxes (mirror of slowfast/datasets/transform.py:42-294).
Every function takes frames [T,C,H,W] on ANY device (the arithmetic is plain torch: the same call augments on the GPU
when the decoded clip already lives there) and boxes [..., 4] xyxy in pixels as a numpy array or a tensor, and draws its
random numbers with the reference's own numpy calls in the reference's order (the resized crop also with Python's
`random`, as the reference does)."""
import math
import random

import numpy as np
import torch


def random_short_side_scale_jitter(images, min_size, max_size, boxes=None, inverse_uniform_sampling=False):
    """transform.py:42-96: resize so that the short side is a uniformly drawn size; boxes scale with it."""
    if inverse_uniform_sampling:
        size = int(round(1.0 / np.random.uniform(1.0 / max_size, 1.0 / min_size)))
    else:
        size = int(round(np.random.uniform(min_size, max_size)))
    height, width = images.shape[2], images.shape[3]
    if (width <= height and width == size) or (height <= width and height == size):
        return images, boxes
    new_width = new_height = size
    if width < height:
        new_height = int(math.floor((float(height) / width) * size))
        if boxes is not None:
            boxes = boxes * float(new_height) / height
    else:
        new_width = int(math.floor((float(width) / height) * size))
        if boxes is not None:
            boxes = boxes * float(new_width) / width
    return torch.nn.functional.interpolate(images, size=(new_height, new_width), mode="bilinear", align_corners=False), boxes


def crop_clip_boxes(boxes, x_offset, y_offset, size):
    """transform.py:98-119: shift into the crop's frame and clip to [0, size]."""
    if isinstance(boxes, np.ndarray):
        cropped, clipf = boxes.copy(), np.clip
    else:
        cropped, clipf = boxes.clone(), torch.clip
    cropped[..., [0, 2]] = clipf(boxes[..., [0, 2]] - x_offset, 0, size)
    cropped[..., [1, 3]] = clipf(boxes[..., [1, 3]] - y_offset, 0, size)
    return cropped


def crop_boxes(boxes, x_offset, y_offset):
    """transform.py:122-138 (no clipping)."""
    cropped = boxes.copy() if isinstance(boxes, np.ndarray) else boxes.clone()
    cropped[..., [0, 2]] = boxes[..., [0, 2]] - x_offset
    cropped[..., [1, 3]] = boxes[..., [1, 3]] - y_offset
    return cropped


def random_crop(images, size, boxes=None):
    """transform.py:141-174.  (The reference returns the bare images when no crop is needed; callers unpack two values,
    so the pair is returned here in that case too.)"""
    if images.shape[2] == size and images.shape[3] == size:
        return images, boxes
    height, width = images.shape[2], images.shape[3]
    y_offset = int(np.random.randint(0, height - size)) if height > size else 0
    x_offset = int(np.random.randint(0, width - size)) if width > size else 0
    cropped = images[:, :, y_offset:y_offset + size, x_offset:x_offset + size]
    return cropped, (crop_clip_boxes(boxes, x_offset, y_offset, size) if boxes is not None else None)


def horizontal_flip(prob, images, boxes=None):
    """transform.py:177-209: x0' = W - x1 - 1, x1' = W - x0 - 1."""
    flipped = None if boxes is None else (boxes.copy() if isinstance(boxes, np.ndarray) else boxes.clone())
    if np.random.uniform() < prob:
        images = images.flip((-1))
        if images.dim() not in (3, 4):
            raise NotImplementedError("Dimension does not supported")
        width = images.shape[-1]
        if boxes is not None:
            flipped[..., [0, 2]] = width - boxes[..., [2, 0]] - 1
    return images, flipped


def uniform_crop(images, size, spatial_idx, boxes=None, scale_size=None):
    """transform.py:212-272: left / centre / right (or top / centre / bottom) crop of the test views."""
    assert spatial_idx in [0, 1, 2]
    ndim = images.dim()
    if ndim == 3:
        images = images.unsqueeze(0)
    height, width = images.shape[2], images.shape[3]
    if scale_size is not None:
        if width <= height:
            width, height = scale_size, int(height / width * scale_size)
        else:
            width, height = int(width / height * scale_size), scale_size
        images = torch.nn.functional.interpolate(images, size=(height, width), mode="bilinear", align_corners=False)
    y_offset = int(math.ceil((height - size) / 2))
    x_offset = int(math.ceil((width - size) / 2))
    if height > width:
        if spatial_idx == 0:
            y_offset = 0
        elif spatial_idx == 2:
            y_offset = height - size
    else:
        if spatial_idx == 0:
            x_offset = 0
        elif spatial_idx == 2:
            x_offset = width - size
    cropped = images[:, :, y_offset:y_offset + size, x_offset:x_offset + size]
    cropped_boxes = crop_clip_boxes(boxes, x_offset, y_offset, size) if boxes is not None else None
    if ndim == 3:
        cropped = cropped.squeeze(0)
    return cropped, cropped_boxes


def clip_boxes_to_image(boxes, height, width):
    """transform.py:275-294."""
    clipped = boxes.copy()
    clipped[:, [0, 2]] = np.minimum(width - 1.0, np.maximum(0.0, boxes[:, [0, 2]]))
    clipped[:, [1, 3]] = np.minimum(height - 1.0, np.maximum(0.0, boxes[:, [1, 3]]))
    return clipped


def _get_param_spatial_crop(scale, ratio, height, width, num_repeat=10, log_scale=True, switch_hw=False):
    """transform.py:520-559: (i, j, h, w) of an Inception-style crop.  Per attempt: Python's random.uniform for the area
    share and for the (log-)aspect ratio, ONE np.random.uniform() (the reference evaluates it on the left of
    `and switch_hw`, so it is drawn whether or not it is used: leaving it out would shift every later flip), and two
    random.randint for an accepted rectangle; after num_repeat rejected attempts the central crop."""
    for _ in range(num_repeat):
        area = height * width
        target_area = random.uniform(*scale) * area
        if log_scale:
            log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
            aspect_ratio = math.exp(random.uniform(*log_ratio))
        else:
            aspect_ratio = random.uniform(*ratio)
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if np.random.uniform() < 0.5 and switch_hw:
            w, h = h, w
        if 0 < w <= width and 0 < h <= height:
            i = random.randint(0, height - h)
            j = random.randint(0, width - w)
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def resized_crop_boxes(boxes, i, j, h, w, target_height, target_width):
    """transform.py:596-599: boxes into the frame of the crop (i, j, h, w), clipped to it, scaled to the target size."""
    boxes = crop_boxes(boxes, j, i)
    boxes[..., [0, 2]] = np.clip(boxes[..., [0, 2]], 0, w) * float(target_width) / w
    boxes[..., [1, 3]] = np.clip(boxes[..., [1, 3]], 0, h) * float(target_height) / h
    return boxes


def random_resized_crop(images, target_height, target_width, scale=(0.8, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), boxes=None):
    """transform.py:562-602: a crop of random area share `scale` and aspect ratio `ratio`, resized to the target size;
    numpy boxes follow it.  Returns images, or (images, boxes) when boxes are given.  (random_resized_crop_with_shift is
    not mirrored: the reference forbids it with boxes.)"""
    height, width = images.shape[2], images.shape[3]
    i, j, h, w = _get_param_spatial_crop(scale, ratio, height, width)
    ret = torch.nn.functional.interpolate(images[:, :, i:i + h, j:j + w], size=(target_height, target_width),
                                          mode="bilinear", align_corners=False)
    if boxes is not None:
        return ret, resized_crop_boxes(boxes, i, j, h, w, target_height, target_width)
    return ret


def _pil_interp(method):
    """transform.py:606-614: PIL's resample code of an interpolation name (bilinear when unknown)."""
    return {"bicubic": 3, "lanczos": 1, "hamming": 5}.get(method, 2)


def create_random_augment(input_size, auto_augment=None, interpolation="bilinear", with_boxes=False):
    """transform.py:649-684 for device clips: the RandAugment planner of datasets/rand_augment.py for a policy string such as
    "rand-m7-n4-mstd0.5-inc1".  The returned object takes no PIL images: `plan(size, boxes)` draws what the reference would
    draw and `ops.randaug_apply` runs the result (datasets/device_sampling.augment_clips).  with_boxes selects the reference's
    boxes variant, which differs in the draws by nothing; boxes are moved whenever plan() is given some."""
    from .rand_augment import rand_augment_transform
    img_size = input_size[-2:] if isinstance(input_size, tuple) else input_size
    if auto_augment:
        assert isinstance(auto_augment, str)
        img_size_min = min(img_size) if isinstance(img_size, tuple) else img_size
        aa_params = {"translate_const": int(img_size_min * 0.45)}
        if interpolation and interpolation != "random":
            aa_params["interpolation"] = _pil_interp(interpolation)
        if auto_augment.startswith("rand"):
            return rand_augment_transform(auto_augment, aa_params)
    raise NotImplementedError


# ---- the colour stage of the AVA pipeline (transform.py:297-517): frames [T,C,H,W] in BGR order, values in [0,1] ----
def blend(images1, images2, alpha):
    """transform.py:297-310."""
    return images1 * alpha + images2 * (1 - alpha)


def grayscale(images):
    """transform.py:313-332: R 0.299, G 0.587, B 0.114 of a BGR clip, repeated over the three channels."""
    img_gray = images.clone()
    gray_channel = 0.299 * images[:, 2] + 0.587 * images[:, 1] + 0.114 * images[:, 0]
    img_gray[:, 0] = gray_channel
    img_gray[:, 1] = gray_channel
    img_gray[:, 2] = gray_channel
    return img_gray


def color_jitter(images, img_brightness=0, img_contrast=0, img_saturation=0):
    """transform.py:335-367: the enabled ops in a drawn order (one np.random.permutation, then each op's own uniform)."""
    jitter = []
    if img_brightness != 0:
        jitter.append("brightness")
    if img_contrast != 0:
        jitter.append("contrast")
    if img_saturation != 0:
        jitter.append("saturation")
    if len(jitter) > 0:
        order = np.random.permutation(np.arange(len(jitter)))
        for idx in range(0, len(jitter)):
            if jitter[order[idx]] == "brightness":
                images = brightness_jitter(img_brightness, images)
            elif jitter[order[idx]] == "contrast":
                images = contrast_jitter(img_contrast, images)
            elif jitter[order[idx]] == "saturation":
                images = saturation_jitter(img_saturation, images)
    return images


def brightness_jitter(var, images):
    """transform.py:370-386."""
    alpha = 1.0 + np.random.uniform(-var, var)
    return blend(images, torch.zeros_like(images), alpha)


def contrast_jitter(var, images):
    """transform.py:389-406: towards the mean grey of each frame ALONE (dim (1,2,3) of [T,C,H,W])."""
    alpha = 1.0 + np.random.uniform(-var, var)
    img_gray = grayscale(images)
    img_gray[:] = torch.mean(img_gray, dim=(1, 2, 3), keepdim=True)
    return blend(images, img_gray, alpha)


def saturation_jitter(var, images):
    """transform.py:409-425."""
    alpha = 1.0 + np.random.uniform(-var, var)
    return blend(images, grayscale(images), alpha)


def _pca_rgb(alphastd, eigval, eigvec):
    """The draw and the RGB shift of lighting_jitter (transform.py:444-450), in numpy float64 as there."""
    alpha = np.random.normal(0, alphastd, size=(1, 3))
    eig_vec = np.array(eigvec)
    eig_val = np.reshape(eigval, (1, 3))
    return np.sum(eig_vec * np.repeat(alpha, 3, axis=0) * np.repeat(eig_val, 3, axis=0), axis=1)


def lighting_jitter(images, alphastd, eigval, eigvec):
    """transform.py:428-473: AlexNet PCA lighting; the channel at BGR position idx gets rgb[2 - idx]."""
    if alphastd == 0:
        return images
    rgb = _pca_rgb(alphastd, eigval, eigvec)
    out_images = torch.zeros_like(images)
    if images.dim() not in (3, 4):
        raise NotImplementedError(f"Unsupported dimension {images.dim()}")
    for idx in range(images.shape[images.dim() - 3]):
        if images.dim() == 3:
            out_images[idx] = images[idx] + rgb[2 - idx]
        else:
            out_images[:, idx] = images[:, idx] + rgb[2 - idx]
    return out_images


def color_normalization(images, mean, stddev):
    """transform.py:476-517: (x - mean[idx]) / stddev[idx] by channel position."""
    if images.dim() not in (3, 4):
        raise NotImplementedError(f"Unsupported dimension {images.dim()}")
    assert len(mean) == images.shape[images.dim() - 3], "channel mean not computed properly"
    assert len(stddev) == images.shape[images.dim() - 3], "channel stddev not computed properly"
    out_images = torch.zeros_like(images)
    for idx in range(len(mean)):
        if images.dim() == 3:
            out_images[idx] = (images[idx] - mean[idx]) / stddev[idx]
        else:
            out_images[:, idx] = (images[:, idx] - mean[idx]) / stddev[idx]
    return out_images


def color_plan(brightness, contrast, saturation, alphastd, eigval, eigvec):
    """What color_jitter(brightness, contrast, saturation) followed by lighting_jitter(alphastd, eigval, eigvec) would do,
    without touching a pixel: consumes exactly their draws in their order and returns the fields of a focus_clip_color
    record -- op (kinds 0 brightness, 1 contrast, 2 saturation in the applied order), alpha (1 + the op's uniform) and shift
    BY BGR POSITION (position idx gets rgb[2 - idx]; zeros for alphastd == 0).  brightness = contrast = saturation = 0 plans
    no op and draws nothing for them (the PCA-only configuration)."""
    kinds = [k for k, var in ((0, brightness), (1, contrast), (2, saturation)) if var != 0]
    var = {0: brightness, 1: contrast, 2: saturation}
    op, alpha = [], []
    if kinds:
        order = np.random.permutation(np.arange(len(kinds)))
        for idx in range(len(kinds)):
            k = kinds[order[idx]]
            op.append(k)
            alpha.append(1.0 + np.random.uniform(-var[k], var[k]))
    shift = [0.0, 0.0, 0.0]
    if alphastd != 0:
        rgb = _pca_rgb(alphastd, eigval, eigvec)
        shift = [float(rgb[2 - idx]) for idx in range(3)]
    return dict(op=op, alpha=alpha, shift=shift)
