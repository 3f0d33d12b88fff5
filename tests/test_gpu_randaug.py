"""csrc/randaug.hip by the C ABI and by the operators above it, bit for bit against the numpy twin of tests/randaug_ref.py, which
tests/test_randaug_ref_cpu.py holds bit-equal to the reference's own outputs (tests/golden/randaug.npz).  No tolerance
anywhere: the twin fixes integer tables, separately rounded fp32 blends and fp64 coordinates and filters, and the kernels
compute the same expressions in the same order, bicubic included.

Shapes: the fixture's frames (24x32, 37x53, 64x48: rows that end mid-run, one to three apply workgroups), every op and argument
of the fixture as ONE mixed-size batch with row strides above 3 W and canaries around every buffer, and one 240x427 frame
(13 stats workgroups and 101 apply workgroups per frame; 427 is odd, so rows start off a dword boundary and end mid-run)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import randaug_ref as rr
from focus_amd import _lib, ops
from focus_amd.slowfast.config.defaults import get_cfg
from focus_amd.slowfast.datasets import device_sampling as ds
from focus_amd.slowfast.datasets import transform

pytestmark = pytest.mark.gpu

CANARY = 0xA5
STAT_WORDS = ops.RANDAUG_STAT_WORDS


@pytest.fixture(scope="module")
def z():
    return rr.fixture()


@pytest.fixture(scope="module")
def imgs():
    return rr.frames()


@pytest.fixture(scope="module")
def big():
    """One 240x427 frame: smooth gradients plus noise, so the histogram is wide and the affine taps differ."""
    rng = np.random.RandomState(7)
    y, x = np.mgrid[0:240, 0:427]
    base = np.stack([(x * 255) // 426, (y * 255) // 239, ((x + 2 * y) * 255) // 904], -1)
    return np.clip(base * 0.7 + rng.randint(0, 70, base.shape) + 10, 0, 255).astype(np.uint8)


def record(fn, args, resample, H, W):
    """The descriptor fields of a reference function at `args` on an H x W frame: (op, farg, iarg, resample, coef)."""
    op = rr.OP_OF_FN[fn]
    farg = float(args[0]) if args and op in (rr.BRIGHTNESS, rr.COLOR, rr.CONTRAST, rr.SHARPNESS) + rr.AFFINE else 0.0
    iarg = int(args[0]) if args and op in (rr.POSTERIZE, rr.SOLARIZE, rr.SOLARIZE_ADD) else 0
    coef = rr.coefficients(op, farg, W, H) if op in rr.AFFINE else None
    if op in rr.AFFINE and coef is None:
        op = rr.COPY                                              # PIL's plain copy
    return op, farg, iarg, resample or rr.BILINEAR, coef


def run_layer(frames, recs, pad=(0, 0)):
    """One focus_randaug_layer call on explicit descriptors.  frames: uint8 [H,W,3] arrays; recs: record() tuples; pad: extra
    bytes per source / destination row.  Every buffer sits in a canary frame.  -> (outputs, workspace words per stats frame);
    asserts that nothing outside the destination pixels and nothing of the sources was written."""
    n = len(frames)
    items = np.zeros(n, dtype=ops._randaug_item_dtype())
    srcs, dsts, slots = [], [], []
    for k, (f, (op, farg, iarg, rs, coef)) in enumerate(zip(frames, recs)):
        H, W = f.shape[:2]
        ss, dstride = 3 * W + pad[0], 3 * W + pad[1]
        s = torch.full((H + 2, ss), CANARY, dtype=torch.uint8)
        s[1:-1, :3 * W] = torch.from_numpy(f.reshape(H, 3 * W))
        s, d = s.cuda(), torch.full((H + 2, dstride), CANARY, dtype=torch.uint8, device="cuda")
        srcs.append(s)
        dsts.append(d)
        it = items[k]
        it["src"], it["src_stride"], it["dst"], it["dst_stride"] = s.data_ptr() + ss, ss, d.data_ptr() + dstride, dstride
        it["H"], it["W"], it["op"], it["farg"], it["iarg"], it["resample"], it["stats_off"] = H, W, op, farg, iarg, rs, -1
        it["fill"][:3] = rr.FILL
        if coef is not None:
            it["coef"] = coef
        if op in rr.NEEDS_STATS:
            it["stats_off"] = len(slots) * STAT_WORDS
            slots.append(k)
    L = _lib.lib()
    ws_bytes = L.focus_randaug_workspace_bytes(len(slots))
    assert ws_bytes == len(slots) * STAT_WORDS * 4
    ws = torch.zeros(max(ws_bytes // 4, 2), dtype=torch.int32, device="cuda")
    table = torch.from_numpy(items.view(np.uint8)).cuda()
    before = [s.clone() for s in srcs]
    status = L.focus_randaug_layer(ctypes.c_void_p(table.data_ptr()), n, max(f.shape[0] for f in frames),
                                   max(f.shape[1] for f in frames), int(bool(slots)), ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == 0
    outs = []
    for f, s, b, d in zip(frames, srcs, before, dsts):
        H, W = f.shape[:2]
        assert torch.equal(s, b)                                  # the source is never written
        d = d.cpu().numpy()
        assert (d[0] == CANARY).all() and (d[-1] == CANARY).all() and (d[1:-1, 3 * W:] == CANARY).all()
        outs.append(d[1:-1, :3 * W].reshape(H, W, 3).copy())
    return outs, {k: ws[i * STAT_WORDS:(i + 1) * STAT_WORDS].cpu().numpy() for i, k in enumerate(slots)}


def check_stats(words, frame):
    hist, lsum = rr.stats(frame)
    assert np.array_equal(words[:768].astype(np.int64), hist.reshape(-1))
    assert int(words[768:770].view(np.uint64)[0]) == lsum and not words[770:].any()


@pytest.mark.parametrize("pad", [(0, 0), (5, 7)], ids=["dense", "strided"])
def test_every_fixture_case_equals_the_twin_in_one_mixed_batch(z, imgs, pad):
    """Every op at every argument of the fixture, on every frame it was recorded on, as one call: frames of three sizes, each
    with its own op.  Bit-equal to the twin and so to the reference's recorded output; with a pad the rows of the sources
    start at every alignment and the destinations' canaries show that no byte past 3 W is written."""
    frames, recs, keys = [], [], []
    for fn, arglist in rr.CASES.items():
        for args in arglist:
            for rs in ((rr.BILINEAR, rr.BICUBIC) if rr.OP_OF_FN[fn] in rr.AFFINE else (None,)):
                for name in rr.FRAMES:
                    key = rr.case_key(fn, name, args, rs)
                    if key in z:
                        frames.append(imgs[name])
                        recs.append(record(fn, args, rs, *imgs[name].shape[:2]))
                        keys.append((key, fn, args, rs, name))
    assert len(frames) == 29 * 4 + 4 + 16 * 9
    outs, stats = run_layer(frames, recs, pad)
    bad = 0
    for got, (key, fn, args, rs, name) in zip(outs, keys):
        want = rr.apply_fn(imgs[name], fn, args, rs or rr.BILINEAR)
        assert np.array_equal(want, z[key])
        d = int((got != want).any(-1).sum())
        if d:
            bad += 1
            print(key, "pixels differing", d, "max", int(np.abs(got.astype(int) - want.astype(int)).max()))
    assert bad == 0
    for k, words in stats.items():
        check_stats(words, frames[k])


def test_large_frame_every_op_and_the_stats_words(big):
    """240x427: the histogram and the mean are merged from 13 workgroups and read back exactly; every op class runs over 101
    apply workgroups with rows that start off a dword boundary."""
    H, W = big.shape[:2]
    cases = [("auto_contrast", (), None), ("equalize", (), None), ("invert", (), None), ("posterize", (2,), None),
             ("solarize", (77,), None), ("solarize_add", (38,), None), ("brightness", (1.37,), None), ("color", (0.63,), None),
             ("contrast", (1.9,), None), ("contrast", (0.1,), None), ("sharpness", (1.9,), None), ("sharpness", (0.1,), None),
             ("rotate", (21.0,), rr.BICUBIC), ("rotate", (-21.0,), rr.BILINEAR), ("shear_x", (0.21,), rr.BICUBIC),
             ("shear_y", (-0.21,), rr.BICUBIC), ("translate_x_rel", (0.315,), rr.BICUBIC),
             ("translate_y_rel", (-0.315,), rr.BILINEAR), ("rotate", (0.0,), rr.BICUBIC)]
    outs, stats = run_layer([big] * len(cases), [record(fn, args, rs, H, W) for fn, args, rs in cases], (0, 3))
    for got, (fn, args, rs) in zip(outs, cases):
        want = rr.apply_fn(big, fn, args, rs or rr.BILINEAR)
        d = int((got != want).any(-1).sum())
        print(fn, args, rs, "pixels differing", d)
        assert d == 0, (fn, args, rs)
    assert sorted(stats) == [0, 1, 8, 9]
    for words in stats.values():
        check_stats(words, big)


def test_entry_point_refusals():
    L = _lib.lib()
    NULL, SHAPE, ALIGN, WORKSPACE = -5, -1, -3, -6
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, s = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.focus_randaug_workspace_bytes(0) == 0 and L.focus_randaug_workspace_bytes(3) == 3 * STAT_WORDS * 4
    assert L.focus_randaug_layer(None, 1, 8, 8, 0, None, 0, s) == NULL
    assert L.focus_randaug_layer(p, 1, 8, 8, 1, None, 0, s) == NULL
    assert L.focus_randaug_layer(p, 0, 8, 8, 0, None, 0, s) == 0
    assert L.focus_randaug_layer(p, 1, 0, 8, 0, None, 0, s) == SHAPE
    assert L.focus_randaug_layer(p, 1, 8, 32769, 0, None, 0, s) == SHAPE
    assert L.focus_randaug_layer(p, 65536, 8, 8, 0, None, 0, s) == SHAPE
    assert L.focus_randaug_layer(p, 1, 8, 8, 1, ctypes.c_void_p(buf.data_ptr() + 4), 4000, s) == ALIGN
    assert L.focus_randaug_layer(p, 1, 8, 8, 1, p, STAT_WORDS * 4 - 4, s) == WORKSPACE
    torch.cuda.synchronize()
    assert not buf.any()


# ---- ops.randaug_apply -----------------------------------------------------------------------------------------------------
def rec_of(fn, args, resample, H, W):
    op, farg, iarg, rs, coef = record(fn, args, resample, H, W)
    return {"op": rr.OP_OF_FN[fn], "farg": farg, "iarg": iarg, "resample": (rs,), "coef": coef, "fill": rr.FILL}


def test_four_layer_plans_on_a_mixed_batch(imgs):
    """Two clips of different size, T = 3, four layers per frame mixing the kernel classes, closed gates (copies) and PIL's
    plain copy (rotation by 0): equal to the twin applied layer by layer; the inputs are not written."""
    a = np.stack([imgs["noise37x53"], imgs["ramp37x53"], imgs["noise37x53"][::-1].copy()])
    b = np.stack([imgs["two64x48"], imgs["const64x48"], np.rot90(imgs["noise24x32"], 1).copy().repeat(2, 0).repeat(2, 1)[:64, :48]])
    plans = []
    for clip in (a, b):
        H, W = clip.shape[1:3]
        r = lambda fn, args=(), rs=None: rec_of(fn, args, rs, H, W)
        plans.append([
            [r("equalize"), r("rotate", (21.0,), rr.BICUBIC), None, r("contrast", (1.37,))],
            [None, None, None, None],
            [r("sharpness", (1.9,)), r("auto_contrast"), r("shear_x", (-0.21,), rr.BILINEAR), r("rotate", (0.0,), rr.BICUBIC)]])
    dev = [torch.from_numpy(c).cuda() for c in (a, b)]
    outs = ops.randaug_apply(dev, plans)
    torch.cuda.synchronize()
    for clip, d, o, pl in zip((a, b), dev, outs, plans):
        assert np.array_equal(d.cpu().numpy(), clip) and o.data_ptr() != d.data_ptr()
        assert o.shape == d.shape and o.dtype == torch.uint8 and o.is_contiguous()
        for t in range(3):
            assert np.array_equal(o[t].cpu().numpy(), rr.apply_plan(clip[t], pl[t])), t
    # one and two layers: the other parities of the ping-pong
    for depth in (1, 2):
        short = [[fr[:depth] for fr in pl] for pl in plans]
        for clip, o, pl in zip((a, b), ops.randaug_apply(dev, short), short):
            for t in range(3):
                assert np.array_equal(o[t].cpu().numpy(), rr.apply_plan(clip[t], pl[t])), (depth, t)
    # a strided view of a wider decode buffer is taken as it is
    wide = torch.from_numpy(np.concatenate([a, a[:, :, ::-1]], 2).copy()).cuda()
    out = ops.randaug_apply([wide[:, :, :53]], [plans[0]])[0]
    assert torch.equal(out, outs[0])


def aug_cfg(per_frame=True, interpolation="bicubic"):
    cfg = get_cfg()
    cfg.merge_from_list(["AUG.ENABLE", "True", "AUG.AA_TYPE", rr.POLICY, "AUG.DIFFERENT_AUG_PER_FRAME", str(per_frame),
                         "AUG.INTERPOLATION", interpolation, "AUG.RE_PROB", "0.0", "AUG.COLOR_JITTER", "0.0"])
    return cfg


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def test_augment_clips_reproduces_the_reference_from_its_recorded_seeds(z, imgs):
    """The shipped AUG block on a one-frame clip from each seed of the fixture: the frame the reference's own transform
    returned through PIL, bit for bit (the planner draws what it drew, the kernels compute what PIL computed)."""
    frame = imgs["noise24x32"]
    clip = torch.from_numpy(frame[None]).cuda()
    for seed in z["policy.shipped.seeds"]:
        seed_all(int(seed))
        out, boxes = ds.augment_clips(aug_cfg(), [clip], None)
        assert boxes is None and np.array_equal(out[0][0].cpu().numpy(), z["policy.shipped.%d.frame" % seed]), seed
    for seed in z["policy.random.seeds"]:
        seed_all(int(seed))
        out, _ = ds.augment_clips(aug_cfg(interpolation="random"), [clip], None)
        assert np.array_equal(out[0][0].cpu().numpy(), z["policy.random.%d.frame" % seed]), seed


@pytest.mark.parametrize("per_frame", [True, False])
def test_augment_clips_on_a_batch_with_boxes(imgs, per_frame):
    """Two clips of different size with boxes: the planner replayed from the same seed gives the plans and the boxes, the twin
    the pixels.  Per frame a fresh transform draws for every frame; otherwise the clip's frames share one plan."""
    a = np.stack([imgs["noise37x53"], imgs["ramp37x53"], imgs["noise37x53"][:, ::-1].copy()])
    b = np.stack([imgs["noise24x32"], imgs["noise24x32"][::-1].copy(), imgs["noise24x32"][:, ::-1].copy()])
    boxes = [np.array([[[5.0, 4.0, 30.0, 20.0], [0.0, 0.0, 0.0, 0.0]]] * 3, dtype=np.float32),
             np.array([[[2.0, 3.0, 20.0, 15.0], [10.0, 1.0, 31.0, 23.0]]] * 3, dtype=np.float32)]
    cfg = aug_cfg(per_frame, "random" if not per_frame else "bicubic")
    seed_all(11)
    out, moved = ds.augment_clips(cfg, [torch.from_numpy(c).cuda() for c in (a, b)], boxes)
    seed_all(11)
    changed = 0
    for clip, bx, o, m in zip((a, b), boxes, out, moved):
        T, H, W = clip.shape[:3]
        make = lambda: transform.create_random_augment((H, W), rr.POLICY, cfg.AUG.INTERPOLATION, with_boxes=True)
        if per_frame:
            plans = [make().plan((W, H), bx[[t]]) for t in range(T)]
            want_boxes = np.concatenate([p[1] for p in plans])
            layers = [p[0] for p in plans]
        else:
            shared, want_boxes = make().plan((W, H), bx, T)
            layers = [[None if r is None else dict(r, resample=(r["resample"][t],)) for r in shared] for t in range(T)]
        assert m.shape == bx.shape and np.array_equal(m, want_boxes)
        assert clip is b or not m[:, 1].any()                     # the all-zero row of the first clip stays zero
        for t in range(T):
            want = rr.apply_plan(clip[t], layers[t])
            assert np.array_equal(o[t].cpu().numpy(), want), t
            changed += int(not np.array_equal(want, clip[t]))
    assert changed >= 4


def test_augmented_clips_feed_the_sampler(imgs):
    """End to end: sample_clips(cfg, *augment_clips(...)) gives the model's input shape and finite values."""
    cfg = aug_cfg()
    cfg.DATA.TRAIN_CROP_SIZE, cfg.DATA.TRAIN_JITTER_SCALES = 16, [20, 24]
    cfg.MODEL.MODEL_NAME, cfg.TRAIN.MIXED_PRECISION = "Motionformer", False
    clips = [torch.from_numpy(np.stack([imgs["noise37x53"]] * 2)).cuda(), torch.from_numpy(np.stack([imgs["noise24x32"]] * 2)).cuda()]
    boxes = [np.array([[[5.0, 4.0, 30.0, 20.0]]] * 2, dtype=np.float32), np.array([[[2.0, 3.0, 20.0, 15.0]]] * 2, dtype=np.float32)]
    seed_all(5)
    inputs, ob = ds.sample_clips(cfg, *ds.augment_clips(cfg, clips, boxes))
    assert inputs.shape == (2, 3, 2, 16, 16) and inputs.dtype == torch.float32 and bool(torch.isfinite(inputs).all())
    assert ob.shape == (2, 2, 1, 4) and np.isfinite(np.asarray(ob)).all()
