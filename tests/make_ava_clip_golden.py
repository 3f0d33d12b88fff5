"""TEST INFRASTRUCTURE: writes tests/golden/ava_clip.npz from the reference's own datasets/transform.py (loaded file by file
like tests/make_clip_sampling_golden.py).  Runs only where the reference tree is present:
    python tests/make_ava_clip_golden.py
The fixture is data only: two small uint8 BGR clips of different sizes whose frames differ strongly in brightness, their
normalised boxes, mean / std, the PCA tables, and per case of ava_clip_ref.CASES the seed (np.random.seed), the fp32 frames
[3,T,S,S] and the boxes that the body of Ava._images_and_boxes_preprocessing (ava_dataset.py:268-365, restated call by call
below: the class itself needs frame lists on disk) makes of them, and the np.random.uniform() drawn right after it, which
pins the number of draws consumed.  Seeds of the six full-colour cases are searched for the wanted op order and flip.  At
the end every mutant of ava_clip_ref must leave the derived bound on some case, the first five on the case named for them."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ava_clip_ref as ar  # noqa: E402
from make_clip_sampling_golden import load_reference  # noqa: E402


def make_clip(g, T, H, W):
    """Ramps plus noise, channels unlike each other, and every frame at another brightness (x 1, 0.55, 0.25, ...): the mean
    grey of one frame is far from the clip's."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = torch.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 11 + 40) % 256, (255 - xx * 5 - yy * 4) % 256], -1).float()
    gain = torch.tensor([1.0, 0.55, 0.25, 0.8])[:T, None, None, None]
    clip = (base[None] + torch.randint(-30, 31, (T, H, W, 3), generator=g)) * gain
    return clip.clamp(0, 255).to(torch.uint8)


def make_boxes(g, n):
    """Normalised xyxy boxes; the first leaves the frame on two sides (clip_boxes_to_image), the last is very thin."""
    xy = torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.5
    wh = torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.4 + 0.08
    b = torch.cat([xy, xy + wh], -1).numpy()
    b[0] = [-0.02, 0.1, 0.6, 1.03]
    b[-1] = [0.5, 0.05, 0.505, 0.95]
    return b


def preprocess(tf, imgs, boxes, split, cfg, log):
    """ava_dataset.py:268-365 with self._* read from cfg as Ava.__init__ does (ava_dataset.py:28-52); imgs uint8 [T,3,H,W]."""
    crop_size = cfg.DATA.TRAIN_CROP_SIZE if split == "train" else cfg.DATA.TEST_CROP_SIZE
    imgs = imgs.float()
    imgs = imgs / 255.0
    height, width = imgs.shape[2], imgs.shape[3]
    boxes[:, [0, 2]] *= width
    boxes[:, [1, 3]] *= height
    boxes = tf.clip_boxes_to_image(boxes, height, width)
    if split == "train":
        imgs, boxes = tf.random_short_side_scale_jitter(imgs, min_size=cfg.DATA.TRAIN_JITTER_SCALES[0],
                                                        max_size=cfg.DATA.TRAIN_JITTER_SCALES[1], boxes=boxes)
        imgs, boxes = tf.random_crop(imgs, crop_size, boxes=boxes)
        before = imgs
        imgs, boxes = tf.horizontal_flip(0.5, imgs, boxes=boxes)
        log.append("flip" if imgs is not before else "noflip")
    elif split == "val":
        imgs, boxes = tf.random_short_side_scale_jitter(imgs, min_size=crop_size, max_size=crop_size, boxes=boxes)
        imgs, boxes = tf.uniform_crop(imgs, size=crop_size, spatial_idx=1, boxes=boxes)
        if cfg.AVA.TEST_FORCE_FLIP:
            imgs, boxes = tf.horizontal_flip(1, imgs, boxes=boxes)
    else:
        raise NotImplementedError(split)
    if split == "train" and cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION:
        if not cfg.AVA.TRAIN_PCA_JITTER_ONLY:
            imgs = tf.color_jitter(imgs, img_brightness=0.4, img_contrast=0.4, img_saturation=0.4)
        imgs = tf.lighting_jitter(imgs, alphastd=0.1, eigval=np.array(cfg.DATA.TRAIN_PCA_EIGVAL).astype(np.float32),
                                  eigvec=np.array(cfg.DATA.TRAIN_PCA_EIGVEC).astype(np.float32))
    imgs = tf.color_normalization(imgs, np.array(cfg.DATA.MEAN, dtype=np.float32), np.array(cfg.DATA.STD, dtype=np.float32))
    if not cfg.AVA.BGR:
        imgs = imgs[:, [2, 1, 0], ...]
    boxes = tf.clip_boxes_to_image(boxes, crop_size, crop_size)
    return imgs, boxes


def run_case(tf, clips, boxes, tag, seed):
    cid, split, _, _ = ar.CASES[tag]
    log = []
    np.random.seed(seed)
    imgs, b = preprocess(tf, clips[cid].permute(0, 3, 1, 2), boxes[cid].copy(), split, ar.case_cfg(tag), log)
    return imgs.permute(1, 0, 2, 3).contiguous().numpy(), b, float(np.random.uniform()), log


def main():
    import warnings
    warnings.filterwarnings("ignore", message="To copy construct from a tensor")
    tf = load_reference()[0]
    kinds = {"brightness_jitter": 0, "contrast_jitter": 1, "saturation_jitter": 2}
    order = []
    for name, k in kinds.items():                                 # log the order the reference applies its ops in
        def wrap(var, images, _f=getattr(tf, name), _k=k):
            order.append(_k)
            return _f(var, images)
        setattr(tf, name, wrap)
    g = torch.Generator().manual_seed(20267)
    clips = {"a": make_clip(g, 3, 20, 27), "b": make_clip(g, 3, 24, 17)}
    boxes = {"a": make_boxes(g, 4), "b": make_boxes(g, 3)}
    out = {"clip_a": clips["a"].numpy(), "clip_b": clips["b"].numpy(), "boxes_a": boxes["a"], "boxes_b": boxes["b"],
           "mean": np.array(ar.MEAN, dtype=np.float32), "std": np.array(ar.STD, dtype=np.float32),
           "eigval": np.array(ar.EIGVAL, dtype=np.float32), "eigvec": np.array(ar.EIGVEC, dtype=np.float32)}
    fixed = {"pca_only": 21, "no_color": 22, "val": 23, "val_flip": 24, "val_bgr": 25}
    for i, tag in enumerate(ar.CASES):
        if tag in fixed:
            seed = fixed[tag]
        else:
            want = (list(ar.ORDERS[i]), "flip" if i % 2 else "noflip")
            for seed in range(5000):
                del order[:]
                log = run_case(tf, clips, boxes, tag, seed)[3]
                if (order, log[0]) == want:
                    break
            else:
                raise RuntimeError("no seed found for " + tag)
        del order[:]
        frames, b, nxt, log = run_case(tf, clips, boxes, tag, seed)
        out.update({tag + ".seed": seed, tag + ".frames": frames, tag + ".boxes": b, tag + ".next": nxt})
        print(tag, "seed", seed, "order", order, log, "frames", frames.shape, "|max| %.3f" % np.abs(frames).max())
    np.savez_compressed(ar.GOLDEN, **out)
    print("wrote", ar.GOLDEN, os.path.getsize(ar.GOLDEN), "bytes")
    check_mutants(ar.fixture())


def check_mutants(z):
    worst = {m: {} for m in ar.MUTANTS}
    for tag, (cid, split, crop, ava) in ar.CASES.items():
        clip, p, color, _, nxt = ar.case_plan(z, tag)
        assert nxt == float(z[tag + ".next"]), tag
        S, rev = p["out_h"], not ava.get("BGR", False)
        args = (clip, p, color, S, S, ar.MEAN, ar.STD, ar.GRAY_BGR, rev)
        ref = ar.sample(*args)[0]
        tol = ar.bound(p, color, S, S, ar.MEAN, ar.STD)
        assert ar.ratio(ar.sample(*args, dtype=np.float32)[0], ref, tol) <= 1.0, tag
        assert ar.ratio(z[tag + ".frames"], ref, ar.bound(p, color, S, S, ar.MEAN, ar.STD, any_order=True)) <= 1.0, tag
        for m in ar.MUTANTS:
            worst[m][tag] = ar.ratio(ar.sample(*args, dtype=np.float32, mutant=m)[0], ref, tol)
    for m in ar.MUTANTS:
        print("%-18s" % m, " ".join("%s %.3g" % kv for kv in worst[m].items()))
        assert max(worst[m].values()) > 1.0, m
        if m in ar.MUTANT_CASE:
            assert worst[m][ar.MUTANT_CASE[m]] > 1.0, (m, ar.MUTANT_CASE[m])


if __name__ == "__main__":
    main()
