"""TEST INFRASTRUCTURE: writes tests/golden/mixup.npz from the reference's own slowfast/datasets/mixup.py (it imports only
numpy and torch, so it is loaded as a single file).  Runs only where the reference tree is present:
    python tests/make_mixup_golden.py
The fixture is data only: one small fp32 clip batch, the labels, and per case of mixup_ref.CASES the seed (np.random.seed),
what the reference drew (lam as drawn, lam as returned, the mode, the box) and what its MixUp.__call__ returned (the mixed
clip and the dense target).  Seeds are searched so that each case reaches the branch it is named after."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mixup_ref  # noqa: E402


def load_reference():
    from oracle._ref_loader import REF
    spec = importlib.util.spec_from_file_location("_reference_mixup", os.path.join(REF, "slowfast", "datasets", "mixup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw(ref, m, shape, seed):
    """What the reference's MixUp draws from this seed, by its own functions in its own order:
    (lam drawn, lam returned, use_cutmix, box or None)."""
    np.random.seed(seed)
    lam0, use_cutmix = m._get_mixup_params()
    if lam0 == 1.0 or not use_cutmix:
        return lam0, lam0, use_cutmix, None
    box, lam = ref.get_cutmix_bbox(shape, lam0, correct_lam=m.correct_lam)
    return lam0, float(lam), use_cutmix, tuple(int(v) for v in box)


def wanted(kind, lam0, lam, use_cutmix, box):
    if kind == "none":
        return lam == 1.0 and not use_cutmix
    if kind == "blend":
        return not use_cutmix and lam not in (1.0, 0.5)
    if not use_cutmix or box is None:
        return False
    yl, yh, xl, xh = box
    area = (yh - yl) * (xh - xl)
    if kind == "empty":
        return area == 0 and lam == 1.0
    if kind == "interior":
        return area > 1 and yl > 0 and xl > 0 and yh < mixup_ref.H and xh < mixup_ref.W
    if kind == "clipped":
        return area > 0 and (yl == 0 or xl == 0 or yh == mixup_ref.H or xh == mixup_ref.W) and \
            abs(lam - lam0) > 1e-3 and (xl % 2 == 1 or (xh - xl) % 2 == 1)
    return kind == "cutmix" and area > 0


def main():
    ref = load_reference()
    g = torch.Generator().manual_seed(20267)
    x = torch.randn(4, 3, 2, mixup_ref.H, mixup_ref.W, generator=g)
    labels = np.array([3, 1, 4, 0], dtype=np.int64)                      # labels[i] != labels[B-1-i] for B = 2, 3, 4
    ek = {"verb": np.array([5, 96, 0, 41], dtype=np.int64), "noun": np.array([299, 7, 7, 120], dtype=np.int64)}
    out = {"x": x.numpy(), "labels": labels, "ek.verb": ek["verb"], "ek.noun": ek["noun"]}
    for tag, (B, _kw, kind) in mixup_ref.CASES.items():
        m = ref.MixUp(**mixup_ref.case_args(tag))
        shape = (B,) + tuple(x.shape[1:])
        for seed in range(100000):
            lam0, lam, use_cutmix, box = draw(ref, m, shape, seed)
            if wanted(kind, lam0, lam, use_cutmix, box):
                break
        else:
            raise RuntimeError("no seed found for " + tag)
        np.random.seed(seed)
        xin = x[:B].clone()
        if tag == "ek_dict":
            got, tgt = m(xin, {k: torch.from_numpy(v[:B]) for k, v in ek.items()})
            out.update({tag + ".target." + k: v.numpy() for k, v in tgt.items()})
        else:
            got, tgt = m(xin, torch.from_numpy(labels[:B]))
            out[tag + ".target"] = tgt.numpy()
        assert got is xin and tgt_dtype(tgt) == torch.float32
        out.update({tag + ".seed": seed, tag + ".lam_drawn": np.float64(lam0), tag + ".lam": np.float64(lam),
                    tag + ".cutmix": np.int64(use_cutmix), tag + ".box": np.array(box or (0, 0, 0, 0), dtype=np.int64),
                    tag + ".clip": got.numpy()})
        print(tag, "seed", seed, "lam", lam0, "->", lam, "cutmix", use_cutmix, "box", box)
    np.savez_compressed(mixup_ref.GOLDEN, **out)
    print("wrote", mixup_ref.GOLDEN, os.path.getsize(mixup_ref.GOLDEN), "bytes")


def tgt_dtype(t):
    return next(iter(t.values())).dtype if isinstance(t, dict) else t.dtype


if __name__ == "__main__":
    main()
