"""TEST INFRASTRUCTURE: writes tests/golden/randaug.npz from the reference's own slowfast/datasets/rand_augment.py (it imports
only PIL and numpy, so it is loaded as a single file).  Runs only where the reference tree and PIL are present:
    python tests/make_randaug_golden.py
The fixture is data only.  Per op (randaug_ref.CASES) it holds what the reference's function returned for the frames of
randaug_ref.frames() at each argument and, for the affine ops, both resamples.  Per policy case it holds the seed
(random.seed and np.random.seed), what the reference's rand_augment_transform drew from it -- the index of each chosen op in
its transform list, whether its gate opened, the argument its level map produced, the resample `_check_args_tf` chose -- the
frame it returned and the next draw of both generators afterwards.  Seeds are searched so that every op of the shipped policy
opens at least once and a closed gate occurs; further cases cover the weighted form (w0), `interpolation: random` with an
open affine op, and the non-increasing list."""
import importlib.util
import os
import random
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import randaug_ref as rr  # noqa: E402

POLICY_FRAME = "noise24x32"
# tag -> (config string, interpolation)
POLICIES = {"shipped": (rr.POLICY, "bicubic"), "weighted": (rr.POLICY + "-w0", "bicubic"), "random": (rr.POLICY, "random"),
            "plain": ("rand-m9-n2-mstd0.5", "bilinear")}


def load_reference():
    from oracle._ref_loader import REF
    spec = importlib.util.spec_from_file_location("_reference_rand_augment",
                                                  os.path.join(REF, "slowfast", "datasets", "rand_augment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frames_for(fn, resample):
    """The frames an op is recorded on (the fixture stays small: the second noise frame only where neighbours matter most)."""
    if rr.OP_OF_FN[fn] in rr.AFFINE:
        return rr.FRAMES if resample == rr.BICUBIC else rr.FRAMES[:4]
    return rr.FRAMES if fn == "sharpness" else rr.FRAMES[:4]


def build(ref, config, interpolation, size):
    """The reference's transform as transform.py:649-684 (create_random_augment) builds it, with the ops named."""
    hparams = {"translate_const": int(min(size) * 0.45)}
    if interpolation != "random":
        hparams["interpolation"] = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[interpolation]
    tr = ref.rand_augment_transform(config, hparams)
    names = ref._RAND_INCREASING_TRANSFORMS if "inc1" in config else ref._RAND_TRANSFORMS
    for i, (op, name) in enumerate(zip(tr.ops, names)):
        op._index, op._name = i, name
    return tr, names


def run_policy(ref, tr, img, seed):
    """-> (records [(index, open, arg, resample)], frame, next random.random(), next np.random.random())"""
    log, chosen = [], []
    real_call, real_interp = ref.AugmentOp.__call__, ref._interpolation

    def interp(kwargs):
        r = real_interp(kwargs)
        chosen.append(int(r))
        return r

    def call(self, im):
        rec = [self._index, 0, np.nan, -1]
        fn = self.aug_fn

        def spy(im_, *args, **kw):
            rec[1] = 1
            if args:
                rec[2] = float(args[0])
            n = len(chosen)
            out = fn(im_, *args, **kw)
            if len(chosen) > n:
                rec[3] = chosen[-1]
            return out

        self.aug_fn = spy
        try:
            out = real_call(self, im)
        finally:
            self.aug_fn = fn
        log.append(rec)
        return out

    ref.AugmentOp.__call__, ref._interpolation = call, interp
    try:
        random.seed(seed)
        np.random.seed(seed)
        out = tr(Image.fromarray(img))
        nxt = (random.random(), float(np.random.random()))
    finally:
        ref.AugmentOp.__call__, ref._interpolation = real_call, real_interp
    return log, np.asarray(out), nxt


def main():
    ref = load_reference()
    imgs = rr.frames()
    out = {"frame." + k: v for k, v in imgs.items()}
    for fn, arglist in rr.CASES.items():
        f = getattr(ref, fn)
        for args in arglist:
            for resample in ((rr.BILINEAR, rr.BICUBIC) if rr.OP_OF_FN[fn] in rr.AFFINE else (None,)):
                for name in frames_for(fn, resample):
                    kw = {} if resample is None else {"resample": resample, "fillcolor": ref._FILL}
                    got = np.asarray(f(Image.fromarray(imgs[name]), *args, **kw))
                    assert got.dtype == np.uint8 and got.shape == imgs[name].shape
                    out[rr.case_key(fn, name, args, resample)] = got
    img = imgs[POLICY_FRAME]
    size = (img.shape[1], img.shape[0])
    for tag, (config, interpolation) in POLICIES.items():
        tr, names = build(ref, config, interpolation, size)
        seeds, seen = [], set()
        want = set(names) | {"closed"} if tag == "shipped" else None
        for seed in range(100000):
            log, frame, nxt = run_policy(ref, tr, img, seed)
            opened = {names[r[0]] for r in log if r[1]} | ({"closed"} if any(not r[1] for r in log) else set())
            if tag == "shipped":
                keep = bool(opened - seen)
            elif tag == "random":
                keep = len({r[3] for r in log if r[3] >= 0}) == 2 if not seeds else any(r[3] >= 0 for r in log)
            else:
                keep = len(opened - {"closed"}) >= 2
            if keep:
                seen |= opened
                seeds.append(seed)
                key = "policy.%s.%d." % (tag, seed)
                out[key + "log"] = np.array(log, dtype=np.float64)
                out[key + "frame"] = frame
                out[key + "next"] = np.array(nxt, dtype=np.float64)
                print(tag, seed, [(names[r[0]], r[1], r[2], r[3]) for r in log])
            if (want is not None and seen >= want) or (want is None and len(seeds) == 3):
                break
        else:
            raise RuntimeError("no seeds found for " + tag)
        out["policy.%s.seeds" % tag] = np.array(seeds, dtype=np.int64)
    np.savez_compressed(rr.GOLDEN, **out)
    print("wrote", rr.GOLDEN, os.path.getsize(rr.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
