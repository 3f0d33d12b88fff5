"""TEST INFRASTRUCTURE: writes tests/golden/random_erasing.npz from the reference's own slowfast/datasets/random_erasing.py
(it imports only math, random and torch, so it is loaded as a single file).  Runs only where the reference tree is present:
    python tests/make_random_erasing_golden.py
The fixture is data only: one small fp32 clip [T,C,H,W] and one image [C,H,W], and per case of erase_ref.CASES the seed
(random.seed and torch.manual_seed), what the reference drew (the rectangles with their frame ranges, the attempts each took,
the next random.random() after the call: where it left the generator) and what its RandomErasing.__call__ returned with
device="cpu".  The rectangles are read off the reference's own calls of `random`, which are logged through a stand-in for the
module's `random` global.  Seeds are searched so that each case reaches the branch it is named after."""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import erase_ref  # noqa: E402


def load_reference():
    from oracle._ref_loader import REF
    spec = importlib.util.spec_from_file_location("_reference_random_erasing",
                                                  os.path.join(REF, "slowfast", "datasets", "random_erasing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class LoggedRandom:
    """Python's `random` with a log of (function, arguments, result) of the calls the reference makes."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        fn = getattr(random, name)

        def call(*a):
            r = fn(*a)
            self.log.append((name, a, r))
            return r
        return call


def rectangles(log, kw, n, frame_h, frame_w):
    """The reference's rectangles from its logged draws: a randint right behind the gate is the count, two randints behind a
    pair of uniforms are top and left of a fit (their upper limits give h and w) -> (rows (t0, t1, top, left, h, w), attempts
    per rectangle)."""
    if n is None:
        spans = [(0, 1)]
    else:
        first = n // kw.get("num_splits", 0) if kw.get("num_splits", 0) > 1 else 0
        spans = [(first, n)] if kw.get("cube", True) else [(i, i + 1) for i in range(first, n)]
    rows, tries, gate, k, pairs = [], [], -1, 0, 0
    while k < len(log):
        name, a, drawn = log[k]
        if name == "random":
            gate, pairs = gate + 1, 0
            if k + 1 < len(log) and log[k + 1][0] == "randint":
                k += 1                                                   # the count
        elif name == "uniform":
            assert log[k + 1][0] == "uniform"
            k, pairs = k + 1, pairs + 1
        else:
            assert name == "randint" and log[k + 1][0] == "randint" and a[0] == 0 and log[k + 1][1][0] == 0
            h, w = frame_h - a[1], frame_w - log[k + 1][1][1]
            rows.append(spans[gate] + (drawn, log[k + 1][2], h, w))
            tries.append(pairs)
            k, pairs = k + 1, 0
        k += 1
    assert gate + 1 == len(spans)
    return rows, tries


def run(ref, logged, kw, inp, seed):
    """The reference's call under `seed` -> (output, its rectangles, attempts, the next random.random())."""
    random.seed(seed)
    torch.manual_seed(seed)
    logged.log = []
    x = inp.clone()
    out = ref.RandomErasing(device="cpu", **kw)(x)
    assert out is x
    n = None if x.dim() == 3 else x.shape[0]
    rows, tries = rectangles(logged.log, kw, n, x.shape[-2], x.shape[-1])
    return x, rows, tries, random.random()


def wanted(kind, rows, tries, closed_gates):
    if kind == "closed":
        return not rows
    if kind == "one":
        return len(rows) == 1 and tries == [1] and rows[0][4] > 1 and rows[0][5] > 1 and rows[0][3] % 2 == 1
    if kind == "retry":
        return len(rows) == 1 and tries[0] > 1
    if kind == "two":
        return len(rows) == 2 and all(r[4] > 0 and r[5] > 0 for r in rows)
    if kind == "overlap":
        return len(rows) == 3 and erase_ref.overlaps(rows)
    return kind == "frames" and closed_gates >= 1 and len({r[0] for r in rows}) >= 2 and len(rows) >= 3


def main():
    ref = load_reference()
    logged = LoggedRandom()
    ref.random = logged
    g = torch.Generator().manual_seed(20268)
    clip = torch.randn(erase_ref.T, erase_ref.C, erase_ref.H, erase_ref.W, generator=g)
    image = torch.randn(erase_ref.C, erase_ref.H, erase_ref.W, generator=g)
    out = {"clip": clip.numpy(), "image": image.numpy()}
    for tag, (kw, what, kind) in erase_ref.CASES.items():
        # "view": ssv2.py:444 hands over the permuted view of a [C,T,H,W] clip; the values are the same clip's
        inp = image if what == "image" else clip.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3) if what == "view" else clip
        for seed in range(100000):
            x, rows, tries, nxt = run(ref, logged, kw, inp, seed)
            # the twin's planner must make the reference's draws to the last one
            random.seed(seed)
            mine, my_tries = erase_ref.plan(kw, None if what == "image" else erase_ref.T, erase_ref.H, erase_ref.W, True)
            assert random.random() == nxt and my_tries == tries, (tag, seed)
            assert [list(r) for r in rows] == mine.tolist(), (tag, seed)
            gates = sum(1 for name, _a, _r in logged.log if name == "random")
            closed = gates - len({(r[0], r[1]) for r in rows}) if not kw.get("cube", True) else int(not rows)
            if wanted(kind, mine.tolist(), tries, closed):
                break
        else:
            raise RuntimeError("no seed found for " + tag)
        # the changed elements are the rectangles' (a normal draw or a 0 never equals the clip's value)
        mask = np.zeros(tuple(inp.shape), bool).reshape((-1,) + tuple(inp.shape[-3:]))
        for t0, t1, top, left, h, w in mine.tolist():
            mask[t0:t1, :, top:top + h, left:left + w] = True
        assert np.array_equal((x.numpy() != inp.numpy()).reshape(mask.shape), mask), tag
        out.update({tag + ".seed": np.int64(seed), tag + ".rects": np.array(rows, dtype=np.int64).reshape(-1, 6), tag + ".attempts": np.array(tries, dtype=np.int64),
                    tag + ".next_random": np.float64(nxt), tag + ".out": x.contiguous().numpy()})
        print(tag, "seed", seed, "rects", mine.tolist(), "attempts", tries)
    np.savez_compressed(erase_ref.GOLDEN, **out)
    print("wrote", erase_ref.GOLDEN, os.path.getsize(erase_ref.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
