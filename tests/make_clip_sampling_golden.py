"""TEST INFRASTRUCTURE: writes tests/golden/clip_sampling.npz from the reference's own datasets/transform.py and
datasets/utils.py (loaded file by file like oracle/make_golden.py main_data).  Runs only where the reference tree is present:
    python tests/make_clip_sampling_golden.py
The fixture is data only: two small uint8 clips, their boxes, and per case of clip_ref.CASES the seed (for random.seed AND
np.random.seed) with what the reference's tensor_normalize -> spatial_sampling -> pack_pathway_output (REVERSE_INPUT_CHANNEL
on) and the ssv2.py:337-346 box hand-off make of them."""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import clip_ref  # noqa: E402


def load_reference():
    from oracle import make_golden as mg
    from oracle._ref_loader import _load, _ns
    mods = mg.load_reference(mg._roi_align_tv)
    for n in ("slowfast.datasets", "torchvision.transforms", "torchvision.transforms.functional", "cv2", "slowfast.utils.env"):
        _ns(n)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["slowfast.utils.env"].pathmgr = None
    for stub in ("rand_augment", "boxes_autoaugment", "random_erasing"):
        m = _ns("slowfast.datasets." + stub)
        m.rand_augment_transform = lambda *a, **k: None
        m.RandomErasing = object
    tf = _load("slowfast.datasets.transform", "slowfast/datasets/transform.py")
    du = _load("slowfast.datasets.utils", "slowfast/datasets/utils.py")
    return tf, du, mods["box_ops"]


def make_clip(g, T, H, W):
    """Smooth ramps plus noise: neighbouring pixels differ, and so do the channels."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = torch.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 11 + 40) % 256, (255 - xx * 5 - yy * 4) % 256], -1).float()
    clip = base[None] + torch.arange(T)[:, None, None, None] * 9 + torch.randint(-30, 31, (T, H, W, 3), generator=g)
    return clip.clamp(0, 255).to(torch.uint8)


def make_boxes(g, T, H, W):
    x0 = torch.rand(T, 2, 1, generator=g) * W * 0.5
    y0 = torch.rand(T, 2, 1, generator=g) * H * 0.5
    wh = torch.rand(T, 2, 2, generator=g) * torch.tensor([W * 0.4, H * 0.4]) + 2.0
    b = torch.cat([x0, y0, x0 + wh[..., :1], y0 + wh[..., 1:]], -1).numpy().astype(np.float32)
    b[1, 1] = 0                                                          # an absent object
    b[0, 0] = [W * 0.5, 1.0, W * 0.5 + 0.2, H - 1.0]                     # thinner than 0.05 of the crop after sampling
    return b


def find_seed(tf, kw, H, W, want_flip):
    """The first seed whose resized crop is followed by the wanted flip outcome (the reference's own draws)."""
    for seed in range(1000):
        random.seed(seed)
        np.random.seed(seed)
        tf._get_param_spatial_crop(kw["scale"], kw["aspect_ratio"], H, W)
        if (np.random.uniform() < 0.5) == want_flip:
            return seed
    raise RuntimeError("no seed found")


def main():
    tf, du, bo = load_reference()
    g = torch.Generator().manual_seed(20266)
    clips = {"a": make_clip(g, 3, 20, 27), "b": make_clip(g, 2, 12, 56)}
    boxes = {"a": make_boxes(g, 3, 20, 27), "b": make_boxes(g, 2, 12, 56)}
    out = {"clip_a": clips["a"].numpy(), "clip_b": clips["b"].numpy(), "boxes_a": boxes["a"], "boxes_b": boxes["b"],
           "mean": np.array(clip_ref.MEAN, dtype=np.float32), "std": np.array(clip_ref.STD, dtype=np.float32)}
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(REVERSE_INPUT_CHANNEL=True),
                                MODEL=types.SimpleNamespace(ARCH="mformer", SINGLE_PATHWAY_ARCH=["mformer"],
                                                            MULTI_PATHWAY_ARCH=["slowfast"]))
    seeds = {"rrc_fallback": 3, "jitter": 11, "jitter_inv": 12, "test0": 13, "test1": 13, "test2": 13}
    for tag, (cid, kw) in clip_ref.CASES.items():
        H, W = clips[cid].shape[1:3]
        seed = seeds[tag] if tag in seeds else find_seed(tf, kw, H, W, tag == "rrc_flip")
        random.seed(seed)
        np.random.seed(seed)
        frames = du.tensor_normalize(clips[cid].clone(), clip_ref.MEAN, clip_ref.STD).permute(3, 0, 1, 2)   # ssv2.py: C T H W
        f, b = du.spatial_sampling(frames, boxes=boxes[cid].reshape([-1, 4]).copy(), random_horizontal_flip=True, **kw)
        b = b.reshape(boxes[cid].shape)                                  # the datasets flatten the boxes around this call
        packed = du.pack_pathway_output(cfg, f)[0]
        h, w = packed.shape[-2:]
        bb = b.copy()
        bb[..., [0, 2]] = bb[..., [0, 2]] / w                            # ssv2.py:337-346
        bb[..., [1, 3]] = bb[..., [1, 3]] / h
        bb = np.clip(bb, 0, 1)
        ob = bo.zero_empty_boxes(bo.box_xyxy_to_cxcywh(torch.from_numpy(bb)), mode="cxcywh")
        out.update({tag + ".seed": seed, tag + ".frames": packed.numpy(), tag + ".boxes_px": b, tag + ".orvit_bboxes": ob.numpy()})
        print(tag, "seed", seed, "frames", tuple(packed.shape), "|max|", float(packed.abs().max()))
    np.savez_compressed(clip_ref.GOLDEN, **out)
    print("wrote", clip_ref.GOLDEN, os.path.getsize(clip_ref.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
