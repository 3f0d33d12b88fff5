"""csrc/random_erase.hip by the C ABI and by the layers above it: every element outside the rectangles keeps its bits, the
rectangles hold +0.0 or the twin's normal values (tests/erase_ref.py) within the bound it derives, the last item of a clip wins
an overlap, both layouts and any base alignment give the same numbers; then the mirror RandomErasing class on device tensors
under the seeds of tests/golden/random_erasing.npz, erase_clips, and make_batch with one train_iter step behind it.

Shapes: B=3, T=4, C=3 at 16x16 (rows are whole 16-byte chunks) and 13x19 (odd row starts: every row begins at another
offset inside a chunk), each also from a base one element past a 16-byte address.  The rectangles: width 1 at left=1, one that
ends at column W-1 on frames [1,3), two overlapping items of one clip (the later on frames [2,4) only), a clip with no item."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import erase_ref
import randaug_ref
from conftest import load_golden
from focus_amd import _lib, ops
from focus_amd.slowfast.config.defaults import get_cfg
from focus_amd.slowfast.datasets import device_sampling as ds
from focus_amd.slowfast.datasets.random_erasing import RandomErasing

pytestmark = pytest.mark.gpu

NULL, SHAPE, DTYPE, ALIGN = -5, -1, -2, -3
B, T, C = 3, 4, 3
SIZES = [(16, 16), (13, 19)]
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = {torch.float32: 0x5a5a5a5a, torch.bfloat16: 0x5a5a}          # 1.5e16 in both: no draw reaches it
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
PAD = 64                                                                  # sentinel elements in front of and behind the tensor
S0, S1 = 0x1234abcd, -0x0badf00d


def items_for(H, W):
    """(clip, t0, t1, top, left, h, w) in the order they are applied; clip 1 has none."""
    return [(0, 0, T, 2, 1, 3, 1), (0, 1, 3, 5, W - 6, 4, 6), (2, 0, T, 1, 3, 8, 9), (2, 2, T, 4, 5, 7, W - 5 - 2)]


@functools.lru_cache(maxsize=None)
def reference(H, W, mode):
    """The twin's result for items_for(H, W), computed once: (table rows, written, values fp64, owner), logical [B,C,T,H,W]."""
    rows = erase_ref.table(items_for(H, W))
    return (rows,) + erase_ref.expected((B, C, T, H, W), rows, mode, S0, S1)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def sentinel_tensor(H, W, dtype, layout, shift=0):
    """(whole buffer, the tensor in its physical shape, its LOGICAL [B,C,T,H,W] view), every element the sentinel."""
    n = B * C * T * H * W
    buf = torch.full((PAD + shift + n + PAD,), SENTINEL[dtype], dtype=INT[dtype], device="cuda").view(dtype)
    x = buf[PAD + shift:PAD + shift + n].view((B, C, T, H, W) if layout == "BCTHW" else (B, T, C, H, W))
    return buf, x, (x if layout == "BCTHW" else x.permute(0, 2, 1, 3, 4))


def seed_tensor():
    return torch.tensor([S0, S1], dtype=torch.int32, device="cuda")


def launch(t, layout, rows, per, mode, seed_words, over=()):
    Bx, H, W = t.shape[0], t.shape[3], t.shape[4]
    Cx, Tx = (t.shape[1], t.shape[2]) if layout == "BCTHW" else (t.shape[2], t.shape[1])
    plane = H * W
    sc, st = (Tx * plane, plane) if layout == "BCTHW" else (plane, Cx * plane)
    table = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
    a = dict(x=ptr(t), dtype=_lib.F32 if t.dtype == torch.float32 else _lib.BF16, B=Bx, T=Tx, C=Cx, H=H, W=W, sb=Cx * Tx * plane,
             sc=sc, st=st, items=ptr(table), n=len(rows), per=per, mode=ops.ERASE_MODES.index(mode), seed=ptr(seed_words))
    a.update(over)                                                         # arguments replaced for the refusals
    status = _lib.lib().focus_random_erase(a["x"], a["dtype"], a["B"], a["T"], a["C"], a["H"], a["W"], a["sb"], a["sc"], a["st"],
                                           a["items"], a["n"], a["per"], a["mode"], a["seed"], stream())
    torch.cuda.synchronize()
    return status


def bits(t):
    return t.contiguous().view(INT[t.dtype]).cpu().numpy()


def check_against_twin(logical, buf, H, W, mode, where):
    rows, written, vals, owner = reference(H, W, mode)
    dtype = logical.dtype
    got_bits, got = bits(logical), logical.double().cpu().numpy()
    assert (got_bits[~written] == SENTINEL[dtype]).all(), where + ": wrote outside"
    frame = bits(buf)
    assert (frame[:PAD] == SENTINEL[dtype]).all() and (frame[-PAD:] == SENTINEL[dtype]).all(), where + ": wrote outside the tensor"
    assert (got_bits[written] != SENTINEL[dtype]).all(), where + ": left part of a rectangle"
    if mode == "const":
        assert (got_bits[written] == 0).all(), where                       # +0.0, not -0.0
        return
    tol = erase_ref.BOUND + (erase_ref.bf16_half_ulp(vals) if dtype == torch.bfloat16 else 0.0)
    ratio = (np.abs(got - vals)[written] / np.broadcast_to(tol, vals.shape)[written]).max()
    print("%s %s: max |kernel - twin| = %.3f of the bound" % (where, mode, ratio))
    assert ratio <= 1.0, where
    # the overlap of clip 2's items holds the LATER item's values, which are not the earlier item's
    over = np.zeros_like(written)
    over[2, :, 2:T, 4:9, 5:12] = True
    assert (owner[over] == 3).all() and over.sum() > 0
    if mode == "pixel":
        first = erase_ref.expected((B, C, T, H, W), rows[:3], mode, S0, S1)[1]
        assert (np.abs(got - first)[over] > 100 * erase_ref.BOUND).mean() > 0.99, where


@pytest.mark.parametrize("mode", ops.ERASE_MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("size", SIZES, ids=["16x16", "13x19"])
def test_kernel_writes_the_rectangles_and_nothing_else(size, dtype, mode):
    H, W = size
    rows = reference(H, W, mode)[0]
    assert rows[:, 0].tolist() == [0, 0, 2, 2] and rows[:, 7].tolist() == [0, 1, 0, 1]
    seed = seed_tensor()
    results = {}
    for layout in ("BCTHW", "BTCHW"):
        for shift in (0, 1):
            buf, x, logical = sentinel_tensor(H, W, dtype, layout, shift)
            assert (x.data_ptr() % 16 == 0) == (shift == 0)
            assert launch(x, layout, rows, 2, mode, seed) == 0
            check_against_twin(logical, buf, H, W, mode, "%s shift %d" % (layout, shift))
            results[layout, shift] = bits(logical)
    first = results["BCTHW", 0]
    for key, got in results.items():                                       # one number per logical element, whatever the layout
        assert np.array_equal(got, first), key
    buf, x, logical = sentinel_tensor(H, W, dtype, "BCTHW")                # the same call again: the same bits
    assert launch(x, "BCTHW", rows, 2, mode, seed) == 0 and np.array_equal(bits(logical), first)
    if mode != "const":                                                    # and another seed: other values in the same places
        other = torch.tensor([S0, S1 + 1], dtype=torch.int32, device="cuda")
        buf, x, logical = sentinel_tensor(H, W, dtype, "BCTHW")
        assert launch(x, "BCTHW", rows, 2, mode, other) == 0
        written = reference(H, W, mode)[1]
        assert np.array_equal(bits(logical)[~written], first[~written]) and (bits(logical)[written] != first[written]).mean() > 0.9


def test_rand_mode_has_one_value_per_item_frame_and_channel():
    H, W = SIZES[1]
    rows, written, vals, owner = reference(H, W, "rand")
    buf, x, logical = sentinel_tensor(H, W, torch.float32, "BTCHW")
    assert launch(x, "BTCHW", rows, 2, "rand", seed_tensor()) == 0
    got = logical.cpu().numpy()
    seen = set()
    for k in range(len(rows)):
        clip = rows[k, 0]
        for c in range(C):
            for t in range(rows[k, 1], rows[k, 2]):
                mine = got[clip, c, t][owner[clip, c, t] == k]
                assert mine.size > 0 and (mine == mine[0]).all()
                seen.add(float(mine[0]))
    assert len(seen) == sum(C * (r[2] - r[1]) for r in rows.tolist())


def test_kernel_clamps_what_the_table_gets_wrong():
    """Descriptors the host would refuse: the kernel clamps them to the tensor and skips the empty ones."""
    H, W = SIZES[1]
    bad = np.array([[0, -1, 99, -2, W - 2, 5, 10, 0],                      # frames and rectangle leave the tensor: clamped
                    [B, 0, T, 0, 0, 4, 4, 0], [-1, 0, T, 0, 0, 4, 4, 0],   # no such clip
                    [1, 0, T, 3, 3, 0, 4, 0], [1, 0, T, 3, 3, 4, -4, 0], [1, 2, 2, 3, 3, 4, 4, 0],     # empty
                    [1, 0, T, H, 0, 4, 4, 0], [1, 0, T, 0, W, 4, 4, 0], [1, T, T + 2, 0, 0, 4, 4, 0],   # wholly outside
                    [1, 0, T, 2 ** 31 - 4, 2 ** 31 - 4, 2 ** 31 - 1, 2 ** 31 - 1, 0]], dtype=np.int64).astype(np.int32)
    for dtype in DTYPES:
        buf, x, logical = sentinel_tensor(H, W, dtype, "BCTHW")
        assert launch(x, "BCTHW", bad, 8, "const", seed_tensor()) == 0
        want = np.zeros((B, C, T, H, W), bool)
        want[0, :, :, 0:3, W - 2:W] = True
        got = bits(logical)
        assert (got[want] == 0).all() and (got[~want] == SENTINEL[dtype]).all()
        frame = bits(buf)
        assert (frame[:PAD] == SENTINEL[dtype]).all() and (frame[-PAD:] == SENTINEL[dtype]).all()


def test_every_refused_call_leaves_the_tensor_untouched():
    H, W = SIZES[0]
    rows = reference(H, W, "pixel")[0]
    seed = seed_tensor()
    for dtype in DTYPES:
        buf, x, logical = sentinel_tensor(H, W, dtype, "BCTHW")
        es = x.element_size()
        cases = [(dict(x=None), NULL), (dict(items=None), NULL), (dict(seed=None), NULL), (dict(n=0), 0), (dict(n=-1), 0),
                 (dict(mode=3), SHAPE), (dict(per=0), SHAPE), (dict(per=ops.ERASE_MAX_PER_CLIP + 1), SHAPE), (dict(B=0), SHAPE),
                 (dict(T=0), SHAPE), (dict(C=0), SHAPE), (dict(H=0), SHAPE), (dict(W=32769), SHAPE), (dict(n=65536), SHAPE),
                 (dict(sc=H * W - 1), SHAPE), (dict(st=0), SHAPE), (dict(sb=0), SHAPE), (dict(dtype=_lib.FP8_E4M3), DTYPE),
                 (dict(dtype=9), DTYPE), (dict(x=ptr(x, es // 2)), ALIGN)]
        for over, want in cases:
            assert launch(x, "BCTHW", rows, 2, "pixel", seed, over) == want, over
        assert (bits(buf) == SENTINEL[dtype]).all()
        for bad in (dict(clip=B), dict(t1=T + 1), dict(h=0), dict(left=W - 2), dict(top=-1)):
            with pytest.raises(ValueError):
                ops.random_erase_(x, [dict(dict(clip=0, t0=0, t1=2, top=1, left=1, h=2, w=3), **bad)], "pixel", "BCTHW", seed)
        with pytest.raises(ValueError, match="contiguous"):
            ops.random_erase_(x.permute(0, 2, 1, 3, 4), [dict(clip=0, t0=0, t1=2, top=1, left=1, h=2, w=3)], "pixel", "BTCHW", seed)
        with pytest.raises(ValueError, match="seed"):
            ops.random_erase_(x, [dict(clip=0, t0=0, t1=2, top=1, left=1, h=2, w=3)], "pixel", "BCTHW", seed.cpu())
        assert ops.random_erase_(x, [], "pixel", "BCTHW") is x
        torch.cuda.synchronize()
        assert (bits(buf) == SENTINEL[dtype]).all()


@pytest.mark.parametrize("layout", ["BCTHW", "BTCHW"])
def test_ops_random_erase_is_the_kernel_with_the_hosts_table(layout):
    H, W = SIZES[1]
    a, b, c, d = [dict(zip(ops.ERASE_ITEM_FIELDS, it)) for it in items_for(H, W)]
    items = [c, a, d, b]                                                   # clips interleaved: each clip's own order survives
    for dtype in DTYPES:
        buf, x, logical = sentinel_tensor(H, W, dtype, layout)
        assert ops.random_erase_(x, items, "pixel", layout, seed_tensor()) is x
        torch.cuda.synchronize()
        check_against_twin(logical, buf, H, W, "pixel", "ops " + layout)
    # without a seed the values come from torch's generator: the same torch seed, the same clip
    outs = []
    for _ in range(2):
        torch.manual_seed(7)
        buf, x, logical = sentinel_tensor(H, W, torch.float32, layout)
        ops.random_erase_(x, items, "rand", layout)
        outs.append(bits(logical))
    assert np.array_equal(outs[0], outs[1])
    torch.manual_seed(8)
    buf, x, logical = sentinel_tensor(H, W, torch.float32, layout)
    ops.random_erase_(x, items, "rand", layout)
    assert not np.array_equal(bits(logical), outs[0])


# ---- the mirror class on device tensors ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def z():
    return erase_ref.fixture()


def rect_mask(shape, rects):
    mask = np.zeros(shape, bool).reshape((-1,) + tuple(shape[-3:]))
    for t0, t1, top, left, h, w in np.asarray(rects).tolist():
        mask[t0:t1, :, top:top + h, left:left + w] = True
    return mask.reshape(shape)


@pytest.mark.parametrize("tag", list(erase_ref.CASES))
def test_mirror_on_the_device_erases_the_fixtures_rectangles(z, tag):
    kw, what, _kind = erase_ref.CASES[tag]
    src = torch.from_numpy(z["image" if what == "image" else "clip"].copy()).cuda()
    if what == "view":                                                     # ssv2.py:444: the permuted view of a [C,T,H,W] clip
        x = src.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
        assert not x.is_contiguous()
    else:
        x = src.clone()
    seed = int(z[tag + ".seed"])
    random.seed(seed)
    torch.manual_seed(seed)
    got = RandomErasing(device="cuda", **kw)(x)
    assert got is x and random.random() == float(z[tag + ".next_random"])
    out, before = x.cpu().numpy(), z["image" if what == "image" else "clip"]
    mask = rect_mask(before.shape, z[tag + ".rects"])
    assert np.array_equal(out != before, mask)                             # the changed elements are the fixture's rectangles
    assert np.array_equal(out[~mask], before[~mask])
    if kw["mode"] == "const":
        assert np.array_equal(out, z[tag + ".out"])
    elif mask.any():
        assert np.isfinite(out).all() and np.abs(out[mask]).max() <= erase_ref.R_MAX
        if kw["mode"] == "rand":                                           # one value per rectangle, frame and channel
            t0, t1, top, left, h, w = z[tag + ".rects"][-1].tolist()
            patch = out[t0, 0, top:top + h, left:left + w] if out.ndim == 4 else out[0, top:top + h, left:left + w]
            assert (patch == patch[0, 0]).all()


def test_mirror_refuses_a_device_view_it_cannot_address():
    x = torch.zeros(4, 3, 10, 28, device="cuda")[..., ::2]
    random.seed(1)
    with pytest.raises(ValueError, match="contiguous"):
        RandomErasing(probability=1.0, mode="pixel")(x)


# ---- erase_clips and make_batch --------------------------------------------------------------------------------------
def erase_cfg(model="Motionformer", mixed=False, count=2, mode="pixel", prob=1.0):
    cfg = get_cfg()
    cfg.merge_from_list(["AUG.ENABLE", True, "AUG.RE_PROB", prob, "AUG.RE_MODE", mode, "AUG.RE_COUNT", count,
                         "MODEL.MODEL_NAME", model, "TRAIN.MIXED_PRECISION", mixed])
    return cfg


@pytest.mark.parametrize("model,dtype", [("Motionformer", torch.float32), ("STEVE", torch.bfloat16)])
def test_erase_clips_erases_every_clip_with_the_references_draws(model, dtype):
    Bq, Tq, Hq, Wq = 3, 4, 16, 20
    cfg = erase_cfg(model, dtype == torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    shape = (Bq, 3, Tq, Hq, Wq) if model == "Motionformer" else (Bq, Tq, 3, Hq, Wq)
    x0 = torch.randn(shape, generator=g).to(dtype)
    random.seed(11)
    masks = []
    for b in range(Bq):                                                    # what the reference's transform draws, clip by clip
        rects = erase_ref.plan(dict(probability=1.0, mode="pixel", max_count=2, num_splits=2), Tq, Hq, Wq)
        assert len(rects) >= 1 and (rects[:, 0] == Tq // 2).all()          # RE_COUNT 2: the first half of the frames stays clean
        masks.append(rect_mask((Tq, 3, Hq, Wq), rects))
    nxt = random.random()
    mask = np.stack(masks)
    if model == "Motionformer":
        mask = mask.transpose(0, 2, 1, 3, 4)
    outs = []
    for _ in range(2):
        random.seed(11)
        torch.manual_seed(5)
        x = x0.clone().cuda()
        got = ds.erase_clips(cfg, x)
        assert got is x and random.random() == nxt
        outs.append(x.float().cpu().numpy())
    before = x0.float().numpy()
    changed = outs[0] != before                       # (a bf16 draw can round to the value it replaces: rare, never outside)
    assert not (changed & ~mask).any() and changed[mask].mean() > (0.97 if dtype == torch.bfloat16 else 0.9999)
    assert np.array_equal(outs[0], outs[1])
    assert np.abs(outs[0][mask]).max() <= erase_ref.R_MAX and abs(outs[0][mask].mean()) < 5.0 / np.sqrt(mask.sum())
    cfg.AUG.RE_PROB = 0.0
    x = x0.clone().cuda()
    assert ds.erase_clips(cfg, x) is x and torch.equal(x.cpu(), x0)


def batch_inputs():
    g = np.random.RandomState(0)
    clips = [g.randint(0, 256, (4, 80, 96, 3), dtype=np.uint8), g.randint(0, 256, (4, 72, 100, 3), dtype=np.uint8)]
    boxes = [np.array([[[5.0, 4.0, 60.0, 50.0], [20.0, 10.0, 90.0, 70.0], [1.0, 2.0, 30.0, 40.0]]] * 4, dtype=np.float32)] * 2
    return [torch.from_numpy(c).cuda() for c in clips], boxes


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def test_make_batch_is_the_three_stages_and_feeds_a_training_step():
    from focus_amd import train
    from focus_amd.slowfast.models import build_model
    from focus_amd.slowfast.models.losses import get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    _a, p = load_golden("motionformer_small")
    cfg = erase_cfg(count=1)
    cfg.merge_from_list(["ORVIT.ENABLE", True, "ORVIT.O", 3, "ORVIT.LAYERS", [1], "DATA.TRAIN_CROP_SIZE", 64,
                         "DATA.TRAIN_JITTER_SCALES", [72, 80], "DATA.NUM_FRAMES", 4, "MF.EMBED_DIM", 64, "MF.DEPTH", 3,
                         "MF.NUM_HEADS", 4, "MF.TEMPORAL_RESOLUTION", 2, "MF.USE_MLP", True, "MODEL.NUM_CLASSES", 10,
                         "TRAIN.DATASET", "Ssv2", "NUM_GPUS", 1, "SOLVER.OPTIMIZING_METHOD", "adamw", "SOLVER.BASE_LR", 1e-3,
                         "SOLVER.CLIP_GRAD_L2NORM", 1.0, "AUG.AA_TYPE", randaug_ref.POLICY, "AUG.INTERPOLATION", "bicubic",
                         "AUG.DIFFERENT_AUG_PER_FRAME", True])
    clips, boxes = batch_inputs()
    seed_all(3)
    inputs, ob = ds.make_batch(cfg, clips, boxes)
    seed_all(3)
    aug, moved = ds.augment_clips(cfg, clips, boxes)
    sampled, want_ob = ds.sample_clips(cfg, aug, moved)
    clean = sampled.clone()
    want = ds.erase_clips(cfg, sampled)
    assert inputs.shape == (2, 3, 4, 64, 64) and inputs.dtype == torch.float32 and torch.equal(inputs, want)
    assert torch.equal(ob, want_ob) and ob.shape == (2, 4, 3, 4)
    erased = (inputs != clean).flatten(1).any(1)
    assert bool(erased.all()) and bool(torch.isfinite(inputs).all())      # RE_PROB 1: every clip has a rectangle
    seed_all(3)                                                            # a test view: the sampler alone, nothing drawn for AUG
    view, view_ob = ds.make_batch(cfg, clips, boxes, spatial_idx=1, min_scale=64, max_scale=64, crop_size=64)
    seed_all(3)
    want_view, want_view_ob = ds.sample_clips(cfg, clips, boxes, 1, min_scale=64, max_scale=64, crop_size=64)
    assert torch.equal(view, want_view) and torch.equal(view_ob, want_view_ob)

    m = build_model(cfg)
    m.load_state_dict({k: v.float() for k, v in p.items()})
    m.train()
    opt = construct_optimizer(m, cfg)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    labels = torch.tensor([3, 7]).cuda()
    preds, _labels, loss = train.train_iter(m, opt, loss_fun, [inputs], labels, {"orvit_bboxes": ob.cuda()}, cfg)
    assert preds.shape == (2, 10) and bool(torch.isfinite(preds).all()) and np.isfinite(float(loss.detach()))
    for name, prm in m.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
