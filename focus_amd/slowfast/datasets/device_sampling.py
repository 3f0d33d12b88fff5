"""Clip sampling on the device: decoded uint8 clips and their boxes in, model inputs and `orvit_bboxes` out.

The reference samples a clip on a loader worker (datasets/utils.py:111-188): float conversion, normalisation, a bilinear
resize of the whole frame, a crop, a flip, the channel reversal.  All three of its modes -- short-side jitter + random crop,
random resized crop (the branch every shipped ORViT config takes: AUG.ENABLE with TRAIN_JITTER_SCALES_RELATIVE), the test
views 0/1/2 -- resize a source rectangle to (rh, rw) and take a window of the result, so here the HOST only draws the
reference's random numbers and moves the boxes (`sampling_params`, bit-identical to the reference) and ONE HIP launch
produces the pixels of the whole batch (`ops.clip_sample`).  RandAugment runs in front of it, on the uint8 clips and on the
device too (`augment_clips`: the host draws the reference's numbers and moves the boxes, `ops.randaug_apply` runs the ops),
and random erasing behind it, in place on the sampled batch (`erase_clips`: the host draws the reference's rectangles, ONE
`ops.random_erase_` writes them).  `make_batch` chains the three.  That is every augmentation the reference's SSv2, Kinetics,
EPIC-Kitchens and STEVE datasets apply: AUG.COLOR_JITTER is read by its ImageNet dataset alone (imagenet.py:136).

AVA is the one video dataset that does jitter colours (ava_dataset.py:255-365): normalised boxes in, [K,5] box rows out, and
between /255 and the normalisation transform.color_jitter (brightness, contrast towards each frame's own mean grey,
saturation, in a drawn order) and transform.lighting_jitter (PCA shift).  `sample_ava_clips` is its hand-off: the host plans
(`sampling_params` for the geometry, `transform.color_plan` for the colours, the reference's draws in its order) and
`ops.clip_sample_color` runs the batch in at most two launches (clip_color.hip)."""
import math

import numpy as np
import torch

from ... import ops
from ..utils import box_ops
from . import transform
from .random_erasing import RandomErasing
from .utils import boxes_to_orvit_format


def sampling_params(height, width, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224, random_horizontal_flip=True,
                    inverse_uniform_sampling=False, aspect_ratio=None, scale=None, boxes=None, crop=True):
    """What datasets/utils.py:111-188 `spatial_sampling` would do to a [T,3,height,width] clip, without touching a pixel.
    Consumes exactly the reference's draws for the chosen mode, in its order (numpy's and Python's global generators).
    Returns (params, boxes): params holds the descriptor fields of ops.clip_sample (sy0, sx0, sh, sw, rh, rw, oy0, ox0, flip)
    and out_h, out_w; boxes (numpy xyxy pixels, or None) are the reference's transformed boxes, bit for bit.  crop=False
    (the test views only) stops after the short-side resize: the window is the whole resized frame (AVA's test split without
    AVA.CENTER_CROP_TEST)."""
    assert spatial_idx in [-1, 0, 1, 2]
    p = dict(sy0=0, sx0=0, sh=height, sw=width, rh=height, rw=width, oy0=0, ox0=0, flip=0, out_h=crop_size, out_w=crop_size)
    if spatial_idx == -1 and not (aspect_ratio is None and scale is None):
        # transform.random_resized_crop: the rectangle itself is resized to the crop size
        i, j, h, w = transform._get_param_spatial_crop(scale, aspect_ratio, height, width)
        p.update(sy0=i, sx0=j, sh=h, sw=w, rh=crop_size, rw=crop_size)
        if boxes is not None:
            boxes = transform.resized_crop_boxes(boxes, i, j, h, w, crop_size, crop_size)
    else:
        # transform.random_short_side_scale_jitter: the whole frame is resized (the test views draw their size too)
        if spatial_idx != -1:
            assert len({min_scale, max_scale}) == 1
            inverse_uniform_sampling = False
        if inverse_uniform_sampling:
            size = int(round(1.0 / np.random.uniform(1.0 / max_scale, 1.0 / min_scale)))
        else:
            size = int(round(np.random.uniform(min_scale, max_scale)))
        rh, rw = height, width
        if not ((width <= height and width == size) or (height <= width and height == size)):
            rh = rw = size
            if width < height:
                rh = int(math.floor((float(height) / width) * size))
                if boxes is not None:
                    boxes = boxes * float(rh) / height
            else:
                rw = int(math.floor((float(width) / height) * size))
                if boxes is not None:
                    boxes = boxes * float(rw) / width
        if rh < crop_size or rw < crop_size:
            raise ValueError("a %dx%d frame resized to %dx%d is smaller than the %d crop" % (height, width, rh, rw, crop_size))
        if spatial_idx == -1:                                     # transform.random_crop
            y_offset = x_offset = 0
            if not (rh == crop_size and rw == crop_size):
                if rh > crop_size:
                    y_offset = int(np.random.randint(0, rh - crop_size))
                if rw > crop_size:
                    x_offset = int(np.random.randint(0, rw - crop_size))
        elif not crop:
            p.update(rh=rh, rw=rw, out_h=rh, out_w=rw)
            return p, boxes
        else:                                                     # transform.uniform_crop
            y_offset = int(math.ceil((rh - crop_size) / 2))
            x_offset = int(math.ceil((rw - crop_size) / 2))
            if rh > rw:
                y_offset = {0: 0, 1: y_offset, 2: rh - crop_size}[spatial_idx]
            else:
                x_offset = {0: 0, 1: x_offset, 2: rw - crop_size}[spatial_idx]
        p.update(rh=rh, rw=rw, oy0=y_offset, ox0=x_offset)
        if boxes is not None and not (spatial_idx == -1 and rh == crop_size and rw == crop_size):
            boxes = transform.crop_clip_boxes(boxes, x_offset, y_offset, crop_size)
    if spatial_idx == -1 and random_horizontal_flip:             # transform.horizontal_flip(0.5, ...)
        flipped = None if boxes is None else boxes.copy()
        if np.random.uniform() < 0.5:
            p["flip"] = 1
            if boxes is not None:
                flipped[..., [0, 2]] = crop_size - boxes[..., [2, 0]] - 1
        boxes = flipped
    return p, boxes


def sample_clips(cfg, clips_u8, boxes, spatial_idx=-1, min_scale=None, max_scale=None, crop_size=None, aspect_ratio=None,
                 scale=None, inverse_uniform_sampling=None, random_horizontal_flip=None):
    """The hand-off between decoding and the model for one batch.  clips_u8: list of uint8 [T,H,W,3] CUDA tensors (H, W may
    differ per clip); boxes: per clip a numpy [T,O,4] array of xyxy pixel boxes.  spatial_idx -1 samples for training (the
    random resized crop when scale / aspect_ratio are given or the config carries DATA.TRAIN_JITTER_SCALES_RELATIVE /
    TRAIN_JITTER_ASPECT_RELATIVE, else jitter + crop), 0/1/2 the test views; sizes default to the config's as in ssv2.py:243-276.
    Returns (inputs, orvit_bboxes [B,T,O,4] float32 on the host): inputs [B,3,T,S,S] normalised with DATA.MEAN / DATA.STD and
    channel-reversed per DATA.REVERSE_INPUT_CHANNEL, or for MODEL.MODEL_NAME "STEVE" [B,T,3,S,S] in [0,1]; bf16 under
    TRAIN.MIXED_PRECISION, else fp32.  One H2D copy of the descriptor table, one kernel launch, no device round-trip."""
    data = cfg.DATA
    if spatial_idx == -1:
        lo, hi = data.TRAIN_JITTER_SCALES
        size = data.TRAIN_CROP_SIZE
        if scale is None and aspect_ratio is None and len(getattr(data, "TRAIN_JITTER_SCALES_RELATIVE", [])):
            scale, aspect_ratio = data.TRAIN_JITTER_SCALES_RELATIVE, data.TRAIN_JITTER_ASPECT_RELATIVE
    else:
        lo = hi = size = data.TEST_CROP_SIZE
    min_scale = lo if min_scale is None else min_scale
    max_scale = hi if max_scale is None else max_scale
    crop_size = size if crop_size is None else crop_size
    if inverse_uniform_sampling is None:
        inverse_uniform_sampling = bool(getattr(data, "INV_UNIFORM_SAMPLE", False))
    if random_horizontal_flip is None:
        random_horizontal_flip = data.RANDOM_FLIP
    if len(clips_u8) != len(boxes):
        raise ValueError("sample_clips takes one box array per clip")
    params, out_boxes = [], []
    for clip, b in zip(clips_u8, boxes):
        p, b = sampling_params(int(clip.shape[1]), int(clip.shape[2]), spatial_idx, min_scale, max_scale, crop_size,
                               random_horizontal_flip, inverse_uniform_sampling, aspect_ratio, scale,
                               np.array(b, dtype=np.float32))
        params.append(p)
        out_boxes.append(b)
    dtype = torch.bfloat16 if cfg.TRAIN.MIXED_PRECISION else torch.float32
    if cfg.MODEL.MODEL_NAME == "STEVE":
        inputs = ops.clip_sample(clips_u8, params, crop_size, crop_size, [0.0] * 3, [1.0] * 3, False, dtype, "BTCHW")
    else:
        inputs = ops.clip_sample(clips_u8, params, crop_size, crop_size, data.MEAN, data.STD, data.REVERSE_INPUT_CHANNEL,
                                 dtype, "BCTHW")
    # one hand-off for the batch: boxes_to_orvit_format works box by box, so this is what B calls would give
    return inputs, boxes_to_orvit_format(np.stack(out_boxes), crop_size, crop_size)


GRAY_BGR = (0.114, 0.587, 0.299)                                  # transform.grayscale by BGR position


def ava_plan(cfg, height, width, boxes, split):
    """What ava_dataset.py:268-365 (`_images_and_boxes_preprocessing`, the "pytorch" backend) would do to a [T,3,height,width]
    clip and its normalised boxes [n,4], without touching a pixel.  Consumes the reference's draws in its order: scale, crop y,
    crop x, flip (train; the flip is always drawn, DATA.RANDOM_FLIP is not read there), the one scale draw of val / test and the
    flip draw of AVA.TEST_FORCE_FLIP, then for train under AVA.TRAIN_USE_COLOR_AUGMENTATION the permutation and three alphas
    (unless AVA.TRAIN_PCA_JITTER_ONLY) and the PCA normal.  Returns (params, color, boxes): the fields of ops.clip_sample_color
    (color.shift by BGR position) and the reference's boxes in pixels of the output, bit for bit."""
    data, ava = cfg.DATA, cfg.AVA
    boxes = np.array(boxes)
    boxes[:, [0, 2]] *= width
    boxes[:, [1, 3]] *= height
    boxes = transform.clip_boxes_to_image(boxes, height, width)
    if split == "train":
        lo, hi = data.TRAIN_JITTER_SCALES
        p, boxes = sampling_params(height, width, -1, lo, hi, data.TRAIN_CROP_SIZE, True, boxes=boxes)
    elif split in ("val", "test"):
        size = data.TEST_CROP_SIZE
        # the reference reads self.AVA.CENTER_CROP_TEST in the test split (an AttributeError); cfg.AVA.CENTER_CROP_TEST is meant
        crop = split == "val" or bool(ava.CENTER_CROP_TEST)
        p, boxes = sampling_params(height, width, 1, size, size, size, boxes=boxes, crop=crop)
        if ava.TEST_FORCE_FLIP:                                   # transform.horizontal_flip(1, ...): the draw is made
            flipped = boxes.copy()
            if np.random.uniform() < 1:
                p["flip"] = 1
                flipped[:, [0, 2]] = p["out_w"] - boxes[:, [2, 0]] - 1
            boxes = flipped
    else:
        raise NotImplementedError("{} split not supported yet!".format(split))
    color = dict(op=[], alpha=[], shift=[0.0, 0.0, 0.0])
    if split == "train" and ava.TRAIN_USE_COLOR_AUGMENTATION:
        var = 0 if ava.TRAIN_PCA_JITTER_ONLY else 0.4
        color = transform.color_plan(var, var, var, 0.1, np.array(data.TRAIN_PCA_EIGVAL).astype(np.float32),
                                     np.array(data.TRAIN_PCA_EIGVEC).astype(np.float32))
    return p, color, transform.clip_boxes_to_image(boxes, p["out_h"], p["out_w"])


def sample_ava_clips(cfg, clips_u8, boxes, split, orvit_boxes=None, source_order="bgr"):
    """The hand-off between decoding and the detection model for one AVA batch (ava_dataset.py:255-365 and 404-437).
    clips_u8: list of uint8 [T,H,W,3] CUDA tensors (H, W may differ per clip) in `source_order` "bgr" (what the reference
    decodes) or "rgb"; boxes: per clip a numpy [n_i,4] array of NORMALISED xyxy boxes; orvit_boxes: per clip [T,O,4]
    normalised or None; split: "train" | "val" | "test".  Returns (inputs [B,3,T,S,S], meta): inputs are channel-ordered BGR
    under AVA.BGR, else RGB, bf16 under TRAIN.MIXED_PRECISION; meta["boxes"] fp32 [K,5] (batch index, x1, y1, x2, y2 in output
    pixels), meta["ori_boxes"] [K,5] the untouched normalised boxes, meta["orvit_bboxes"] [B,T,O,4] cxcywh in [0,1] with empty
    boxes zeroed (when orvit_boxes were given).  DATA.MEAN / STD are indexed by BGR position, as in the reference; the grey
    weights and the PCA shift follow the true colours of either source order.  The test split without AVA.CENTER_CROP_TEST
    returns rh x rw frames: every clip of the batch must then resize to one size (ValueError otherwise).  The pixels are
    those of AVA.IMG_PROC_BACKEND "pytorch" under either backend."""
    if source_order not in ("bgr", "rgb"):
        raise ValueError("sample_ava_clips: source_order is bgr or rgb (got %r)" % (source_order,))
    if len(clips_u8) != len(boxes) or (orvit_boxes is not None and len(orvit_boxes) != len(clips_u8)):
        raise ValueError("sample_ava_clips takes one box array (and one ORViT box array) per clip")
    params, colors, det, ori, orv = [], [], [], [], []
    for i, clip in enumerate(clips_u8):
        T, H, W = int(clip.shape[0]), int(clip.shape[1]), int(clip.shape[2])
        b = np.array(boxes[i])
        if b.ndim != 2 or b.shape[1] != 4:
            raise ValueError("sample_ava_clips: clip %d has boxes of shape %s" % (i, b.shape))
        n = b.shape[0]
        ori.append(np.concatenate([np.full((n, 1), float(i)), b], axis=1))
        if orvit_boxes is not None:
            ob = np.asarray(orvit_boxes[i])
            if ob.ndim != 3 or ob.shape[0] != T or ob.shape[2] != 4:
                raise ValueError("sample_ava_clips: clip %d has %d frames and ORViT boxes of shape %s" % (i, T, ob.shape))
            b = np.concatenate([b, ob.reshape(-1, 4)], axis=0)
        p, color, b = ava_plan(cfg, H, W, b, split)
        params.append(p)
        colors.append(color)
        det.append(np.concatenate([np.full((n, 1), float(i)), b[:n]], axis=1))
        if orvit_boxes is not None:
            o = torch.from_numpy(b[n:].reshape(ob.shape))
            o = o / torch.tensor([p["out_w"], p["out_h"], p["out_w"], p["out_h"]]).reshape(1, 1, 4)
            orv.append(box_ops.zero_empty_boxes(box_ops.box_xyxy_to_cxcywh(o), mode="cxcywh").float())
    out_h, out_w = params[0]["out_h"], params[0]["out_w"]
    if any((p["out_h"], p["out_w"]) != (out_h, out_w) for p in params):
        raise ValueError("sample_ava_clips: without AVA.CENTER_CROP_TEST the clips of a batch must resize to one size (got %s)"
                         % sorted({(p["out_h"], p["out_w"]) for p in params}))
    mean, std, gray = list(cfg.DATA.MEAN), list(cfg.DATA.STD), list(GRAY_BGR)
    if source_order == "rgb":                                     # source channel c sits at BGR position 2 - c
        mean, std, gray = mean[::-1], std[::-1], gray[::-1]
        colors = [dict(c, shift=c["shift"][::-1]) for c in colors]
    reverse = (source_order == "bgr") != bool(cfg.AVA.BGR)
    dtype = torch.bfloat16 if cfg.TRAIN.MIXED_PRECISION else torch.float32
    inputs = ops.clip_sample_color(clips_u8, params, colors, out_h, out_w, mean, std, gray, reverse, dtype, "BCTHW")
    meta = {"boxes": torch.from_numpy(np.concatenate(det, axis=0).astype(np.float32)),
            "ori_boxes": torch.from_numpy(np.concatenate(ori, axis=0).astype(np.float32))}
    if orvit_boxes is not None:
        meta["orvit_bboxes"] = torch.stack(orv)
    return inputs, meta


def augment_clips(cfg, clips_u8, boxes=None):
    """The device form of ssv2.py:361-393 (`_aug_frame` up to `_list_img_to_frames`): RandAugment of a batch of decoded clips
    under cfg.AUG.  clips_u8: uint8 [T,H,W,3] CUDA tensors; boxes: None, or per clip a numpy [T,O,4] array of xyxy pixel
    boxes.  Under AUG.DIFFERENT_AUG_PER_FRAME every frame gets a fresh transform and its own draws, as the reference builds
    them; otherwise one transform plans the whole clip (with `interpolation: random` its frames still draw their resample one
    by one).  The draws are the reference's, clip by clip and frame by frame in order; ONE ops.randaug_apply runs the batch.
    Returns (clips_u8, boxes) for sample_clips: new tensors and new box arrays, or the inputs themselves when AUG.ENABLE is
    false or AUG.AA_TYPE is empty.  AUG.RE_PROB belongs to erase_clips; AUG.COLOR_JITTER is not read, as in the reference's video
    datasets (only imagenet.py:136 reads it)."""
    aug = getattr(cfg, "AUG", None)
    aa_type = getattr(aug, "AA_TYPE", "") if aug is not None else ""
    if aug is None or not getattr(aug, "ENABLE", False) or not aa_type:
        return clips_u8, boxes
    if boxes is not None and len(boxes) != len(clips_u8):
        raise ValueError("augment_clips takes one box array per clip")
    interpolation = getattr(aug, "INTERPOLATION", "bicubic")
    per_frame = bool(getattr(aug, "DIFFERENT_AUG_PER_FRAME", False))
    plans, out_boxes = [], []
    for i, clip in enumerate(clips_u8):
        T, H, W = int(clip.shape[0]), int(clip.shape[1]), int(clip.shape[2])
        b = None if boxes is None else np.asarray(boxes[i])
        if b is not None and (b.ndim != 3 or b.shape[0] != T or b.shape[2] != 4):
            raise ValueError("augment_clips: clip %d has %d frames and boxes of shape %s" % (i, T, b.shape))
        make = lambda: transform.create_random_augment((H, W), aa_type, interpolation, with_boxes=b is not None)
        if per_frame:
            frames, moved = [], []
            for t in range(T):
                layers, bt = make().plan((W, H), None if b is None else b[[t]], 1)
                frames.append(layers)
                moved.append(bt)
            b = None if b is None else np.concatenate(moved, axis=0)
        else:
            layers, b = make().plan((W, H), b, T)
            frames = [[None if r is None else dict(r, resample=(r["resample"][t],)) for r in layers] for t in range(T)]
        plans.append(frames)
        out_boxes.append(b)
    return ops.randaug_apply(clips_u8, plans), (None if boxes is None else out_boxes)


def erase_clips(cfg, inputs):
    """The device form of ssv2.py:436-446 (the end of `_aug_frame`; kinetics.py:398-410 and epickitchens.py:347-359 alike):
    RandomErasing of a sampled batch under cfg.AUG, in place.  inputs: what sample_clips returned, [B,3,T,S,S] or for
    MODEL.MODEL_NAME "STEVE" [B,T,3,S,S].  Every clip gets the reference's transform -- RandomErasing(AUG.RE_PROB,
    mode=AUG.RE_MODE, max_count=AUG.RE_COUNT, num_splits=AUG.RE_COUNT) -- and its draws from Python's `random`, clip by clip
    in order; ONE ops.random_erase_ writes the rectangles of the batch.  The fill values come from the build-owned generator,
    seeded from torch's (ops.random_erase_).  Returns `inputs` itself; untouched when AUG.ENABLE is false or AUG.RE_PROB is
    not above 0."""
    aug = getattr(cfg, "AUG", None)
    prob = getattr(aug, "RE_PROB", 0.25) if aug is not None else 0.0
    if aug is None or not getattr(aug, "ENABLE", False) or not prob > 0:
        return inputs
    if inputs.dim() != 5:
        raise ValueError("erase_clips takes the 5-d batch sample_clips returns (got shape %s)" % (tuple(inputs.shape),))
    mode, count = getattr(aug, "RE_MODE", "pixel"), getattr(aug, "RE_COUNT", 1)
    layout = "BTCHW" if cfg.MODEL.MODEL_NAME == "STEVE" else "BCTHW"
    T = int(inputs.shape[1] if layout == "BTCHW" else inputs.shape[2])
    H, W = int(inputs.shape[3]), int(inputs.shape[4])
    items = []
    for b in range(inputs.shape[0]):
        erase = RandomErasing(prob, mode=mode, max_count=count, num_splits=count, device="cpu")
        items += [dict(it, clip=b) for it in erase.plan(T, H, W) if it["h"] > 0 and it["w"] > 0 and it["t0"] < it["t1"]]
    return ops.random_erase_(inputs, items, erase.mode, layout)


def make_batch(cfg, clips_u8, boxes, spatial_idx=-1, **sampling):
    """Decoded uint8 clips and their boxes -> (inputs, orvit_bboxes), every stage on the device.  Training (spatial_idx -1):
    augment_clips -> sample_clips -> erase_clips, what Ssv2._aug_frame does to a clip under AUG.ENABLE (without AUG the first
    and the last return their inputs); the test views 0/1/2: sample_clips alone.  `sampling` goes to sample_clips.  The
    draws are consumed stage by stage, each stage clip by clip."""
    if spatial_idx != -1:
        return sample_clips(cfg, clips_u8, boxes, spatial_idx, **sampling)
    clips_u8, boxes = augment_clips(cfg, clips_u8, boxes)
    inputs, orvit_bboxes = sample_clips(cfg, clips_u8, boxes, spatial_idx, **sampling)
    return erase_clips(cfg, inputs), orvit_bboxes
