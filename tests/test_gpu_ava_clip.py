"""focus_clip_gray_mean / focus_clip_sample_color by the C ABI in guarded buffers, and the AVA sampler above them, against the
fp64 formula of tests/ava_clip_ref.py within the bound derived there.  Shapes are the smallest that reach each hazard: two
clips of different size in one launch, 13x13 outputs (tail run shorter than 8, unaligned rows) and 16x8 outputs (16-byte
stores), and one 40x56 output whose 280 runs need two blocks per frame (the cross-block sum)."""
import ctypes

import numpy as np
import pytest
import torch

import ava_clip_ref as ar
import clip_ref
from focus_amd import _lib, ops
from focus_amd.slowfast.datasets import device_sampling as ds

pytestmark = pytest.mark.gpu

CANARY = -768.0               # exact in bf16 too
PAD = 64
NULL, SHAPE, DTYPE, ALIGN, WORKSPACE = -5, -1, -2, -3, -6
TDT = {_lib.F32: torch.float32, _lib.BF16: torch.bfloat16}
ALPHAS = [1.31, 0.72, 1.18]
SHIFT = [0.021, -0.034, 0.012]
NONE = dict(op=[], alpha=[], shift=[0.0, 0.0, 0.0])


def rec(order, alphas=ALPHAS, shift=SHIFT):
    return dict(op=list(order), alpha=list(alphas[:len(order)]), shift=list(shift))


@pytest.fixture(scope="module")
def sources():
    """name -> (numpy [3,H,W,3], device tensor): the sampler fixture's clip a (81-byte rows) and a 3x40x64 clip whose frames
    differ in brightness."""
    g = torch.Generator().manual_seed(5)
    big = (torch.randint(0, 256, (3, 40, 64, 3), generator=g).float() * torch.tensor([1.0, 0.5, 0.2])[:, None, None, None]).to(torch.uint8)
    a = torch.from_numpy(clip_ref.fixture()["clip_a"])
    return {"a": (a.numpy(), a.cuda()), "big": (big.numpy(), big.cuda())}


def items_table(entries):
    """focus_clip_item records written by hand: (device clip, params) -> int64 [n, 9] on the device."""
    out = np.zeros((len(entries), 9), dtype=np.int64)
    for i, (c, p) in enumerate(entries):
        ints = [c.shape[1], c.shape[2], p["sy0"], p["sx0"], p["sh"], p["sw"], p["rh"], p["rw"], p["oy0"], p["ox0"], p["flip"], 0]
        out[i, :3] = c.data_ptr(), c.stride(1), c.stride(0)
        out[i, 3:] = [ints[2 * k] | (ints[2 * k + 1] << 32) for k in range(6)]
    return torch.from_numpy(out).cuda()


def f3(v):
    arr = (ctypes.c_float * 3)(*v)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Launch:
    """Both entry points on (device clip, params, colour) entries with every device buffer framed by canaries."""

    def __init__(self, entries, out_h, out_w, dtype=_lib.F32, layout="BCTHW", reverse=0, mean=ar.MEAN, std=ar.STD, gray=ar.GRAY_BGR):
        L = _lib.lib()
        self.B, self.T, self.h, self.w = len(entries), entries[0][0].shape[0], out_h, out_w
        B, T, plane = self.B, self.T, out_h * out_w
        self.n = B * 3 * T * plane
        self.buf = torch.full((PAD + self.n + PAD,), CANARY, dtype=TDT[dtype], device="cuda")
        self.fm = torch.full((PAD + B * T + PAD,), CANARY, device="cuda")
        self.ws_bytes = int(L.focus_clip_color_workspace_bytes(B, T, out_h, out_w))
        self.ws = torch.full((PAD + self.ws_bytes // 4 + PAD,), CANARY, device="cuda")
        items = items_table([(c, p) for c, p, _ in entries])
        colors = torch.from_numpy(ops.clip_colors([c for _, _, c in entries], B)).cuda()
        sc, st = (T * plane, plane) if layout == "BCTHW" else (plane, 3 * plane)
        (k1, m), (k2, s), (k3, g) = f3(mean), f3(std), f3(gray)
        self.s_mean = L.focus_clip_gray_mean(ptr(items), ptr(colors), B, T, out_h, out_w, g, ptr(self.fm[PAD:]), ptr(self.ws[PAD:]),
                                             self.ws_bytes, stream())
        self.s_out = L.focus_clip_sample_color(ptr(items), ptr(colors), ptr(self.fm[PAD:]), B, T, out_h, out_w, ptr(self.buf[PAD:]),
                                               3 * T * plane, sc, st, m, s, g, int(reverse), dtype, stream())
        torch.cuda.synchronize()
        res = self.buf[PAD:PAD + self.n].double().cpu().numpy()
        self.res = res.reshape(B, 3, T, out_h, out_w) if layout == "BCTHW" else res.reshape(B, T, 3, out_h, out_w).transpose(0, 2, 1, 3, 4)
        self.means = self.fm[PAD:PAD + B * T].double().cpu().numpy().reshape(B, T)

    def canaries_intact(self):
        ok = True
        for t, n in ((self.buf, self.n), (self.fm, self.B * self.T), (self.ws, self.ws_bytes // 4)):
            ok = ok and bool((t[:PAD].float() == CANARY).all()) and bool((t[PAD + n:].float() == CANARY).all()) and t[PAD + n:].numel() == PAD
        return ok


def check(entries_np, run, dtype=_lib.F32, reverse=0, coords=True, label=""):
    """Pixels and frame means of a Launch against fp64 -> the worst ratios, asserted <= 1."""
    assert run.s_mean == 0 and run.s_out == 0 and run.canaries_intact()
    worst = worst_mean = 0.0
    for b, (src, p, color) in enumerate(entries_np):
        ref, means = ar.sample(src, p, color, run.h, run.w, ar.MEAN, ar.STD, ar.GRAY_BGR, reverse)
        tol = ar.bound(p, color, run.h, run.w, ar.MEAN, ar.STD, ref=ref, bf16=dtype == _lib.BF16, coords=coords)
        worst = max(worst, ar.ratio(run.res[b], ref, tol))
        if ar.CONTRAST in color["op"]:
            worst_mean = max(worst_mean, ar.ratio(run.means[b], means, ar.mean_bound(p, color, run.h, run.w, coords)))
        else:
            assert not run.means[b].any()                        # exactly 0 for a clip without contrast
    print("%s pixels error / bound %.3f, frame mean error / bound %.3f" % (label, worst, worst_mean))
    assert worst <= 1.0 and worst_mean <= 1.0


def pair_params(out_h, out_w):
    """Clip a: a rectangle ending on the last source row and column, upscaled 2.4x, the window at the far end of the resized
    image (second-tap clamp), mirrored.  The big clip: the whole frame downscaled 2.2x, an interior window, not mirrored."""
    pa = dict(sy0=8, sx0=14, sh=12, sw=13, rh=30, rw=31, oy0=30 - out_h, ox0=31 - out_w, flip=1)
    pb = dict(sy0=0, sx0=0, sh=40, sw=64, rh=18, rw=29, oy0=17 - out_h, ox0=7, flip=0)
    return pa, pb


def pair(sources, out_h, out_w, ca, cb):
    pa, pb = pair_params(out_h, out_w)
    dev = [(sources["a"][1], pa, ca), (sources["big"][1], pb, cb)]
    host = [(sources["a"][0], pa, ca), (sources["big"][0], pb, cb)]
    return dev, host


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("layout", ["BCTHW", "BTCHW"])
@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
@pytest.mark.parametrize("out_hw", [(13, 13), (16, 8)])
def test_two_clips_one_launch(sources, out_hw, dtype, layout, reverse):
    out_h, out_w = out_hw
    k = (reverse + 2 * (layout == "BTCHW") + 4 * (dtype == _lib.BF16) + 8 * (out_h == 16)) % 6     # all six orders over the cases
    dev, host = pair(sources, out_h, out_w, rec(ar.ORDERS[k]), rec(ar.ORDERS[(k + 3) % 6], [0.66, 1.27, 1.39], [-0.01, 0.0, 0.03]))
    run = Launch(dev, out_h, out_w, dtype, layout, reverse)
    check(host, run, dtype, reverse, label="%dx%d %s %s reverse %d orders %s %s:" % (
        out_h, out_w, TDT[dtype], layout, reverse, ar.ORDERS[k], ar.ORDERS[(k + 3) % 6]))


@pytest.mark.parametrize("colors", [(NONE, rec((1, 2, 0))), (rec((0, 1, 2)), NONE), (rec((), shift=SHIFT), rec((2, 1))),
                                    (rec((), shift=SHIFT), NONE)], ids=["none+three", "three+none", "pca+two", "pca+none"])
def test_records_without_ops_beside_records_with(sources, colors):
    dev, host = pair(sources, 13, 13, *colors)
    check(host, Launch(dev, 13, 13, _lib.F32, "BCTHW", 1), reverse=1, label="%s | %s:" % (colors[0]["op"], colors[1]["op"]))


@pytest.mark.parametrize("order", [(1, 0, 2), (0, 1, 2), (2, 0, 1)], ids=["first", "middle", "last"])
def test_two_blocks_per_frame(sources, order):
    """40x56: 7 runs x 40 rows = 280 threads, two blocks, whose partials the last-arriving block adds in block order."""
    big_np, big = sources["big"]
    p = dict(sy0=0, sx0=0, sh=40, sw=64, rh=44, rw=70, oy0=2, ox0=9, flip=1)
    color = rec(order)
    assert _lib.lib().focus_clip_color_workspace_bytes(1, 3, 40, 56) == 3 * 3 * 4
    runs = [Launch([(big, p, color)], 40, 56) for _ in range(2)]
    check([(big_np, p, color)], runs[0], label="40x56 contrast %s:" % (order,))
    assert torch.equal(runs[0].buf, runs[1].buf) and torch.equal(runs[0].fm, runs[1].fm)           # the same bits
    twin, means = ar.sample(big_np, p, color, 40, 56, ar.MEAN, ar.STD, ar.GRAY_BGR, 0, dtype=np.float32)
    print("frame means, kernel - twin in its summation order:", runs[0].means[0] - means.astype(np.float64))


def test_two_calls_give_the_same_bits(sources):
    dev, _ = pair(sources, 13, 13, rec((2, 1, 0)), rec((1, 0)))
    a, b = (Launch(dev, 13, 13, _lib.BF16, "BTCHW", 1) for _ in range(2))
    assert torch.equal(a.buf.view(torch.int16), b.buf.view(torch.int16)) and torch.equal(a.fm, b.fm)


def test_refusals_write_nothing(sources):
    L = _lib.lib()
    a_dev = sources["a"][1]
    p = pair_params(13, 13)[0]
    items = items_table([(a_dev, p)])
    colors = torch.from_numpy(ops.clip_colors([rec((1, 0, 2))], 1)).cuda()
    out = torch.full((4096,), CANARY, device="cuda")
    fm = torch.full((64,), CANARY, device="cuda")
    ws = torch.full((64,), CANARY, device="cuda")
    (k1, m), (k2, s), (k3, g) = f3(ar.MEAN), f3(ar.STD), f3(ar.GRAY_BGR)
    need = L.focus_clip_color_workspace_bytes(1, 3, 13, 13)

    def mean_call(it=ptr(items), co=ptr(colors), n=1, T=3, h=13, w=13, gw=g, f=ptr(fm), wsp=ptr(ws), nbytes=need):
        return L.focus_clip_gray_mean(it, co, n, T, h, w, gw, f, wsp, nbytes, None)

    def out_call(it=ptr(items), co=ptr(colors), f=ptr(fm), n=1, T=3, h=13, w=13, o=ptr(out), mm=m, ss=s, gw=g, dt=_lib.F32):
        return L.focus_clip_sample_color(it, co, f, n, T, h, w, o, 3 * T * h * w, T * h * w, h * w, mm, ss, gw, 0, dt, None)

    for kw in (dict(it=None), dict(co=None), dict(gw=None), dict(f=None), dict(wsp=None)):
        assert mean_call(**kw) == NULL, kw
    for kw in (dict(it=None), dict(co=None), dict(f=None), dict(o=None), dict(mm=None), dict(ss=None), dict(gw=None)):
        assert out_call(**kw) == NULL, kw
    assert mean_call(it=None, n=0, h=0) == NULL and out_call(o=None, n=0, dt=7) == NULL            # NULL is judged first
    assert mean_call(n=0) == 0 and mean_call(T=0, h=0) == 0 and out_call(n=-1, h=0, dt=7) == 0    # nothing to do: no launch
    assert mean_call(h=0) == SHAPE and mean_call(w=-2) == SHAPE and mean_call(T=65536) == SHAPE
    assert out_call(h=0) == SHAPE and out_call(w=-2) == SHAPE and out_call(h=0, dt=7) == SHAPE     # the shape before the dtype
    assert mean_call(f=ctypes.c_void_p(fm.data_ptr() + 2)) == ALIGN and mean_call(wsp=ctypes.c_void_p(ws.data_ptr() + 1)) == ALIGN
    assert mean_call(nbytes=need - 1) == WORKSPACE and mean_call(nbytes=0) == WORKSPACE
    assert mean_call(h=40, w=56) == WORKSPACE                                                      # needs three words a frame
    assert out_call(dt=_lib.FP8_E4M3) == DTYPE and out_call(dt=-1) == DTYPE
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((fm == CANARY).all()) and bool((ws == CANARY).all())
    assert mean_call() == 0 and out_call() == 0                   # and the same arguments, accepted, do write
    torch.cuda.synchronize()
    assert bool((fm[:3] != CANARY).all()) and bool((fm[3:] == CANARY).all())
    assert bool((out[:3 * 3 * 169] != CANARY).all()) and bool((out[3 * 3 * 169:] == CANARY).all())
    assert bool((ws[need // 4:] == CANARY).all())


def test_wrapper_matches_the_abi_and_validates_what_the_kernel_cannot(sources):
    a_np, a_dev = sources["a"]
    good = dict(sy0=8, sx0=14, sh=12, sw=13, rh=30, rw=31, oy0=17, ox0=18, flip=1)
    color = rec((2, 1, 0))
    call = lambda **kw: ops.clip_sample_color(**dict(dict(clips=[a_dev], params=[good], colors=[color], out_h=13, out_w=13, mean=ar.MEAN,
                                                          std=ar.STD, gray_w=ar.GRAY_BGR, reverse=True, layout="BTCHW"), **kw))
    out = call()
    assert out.shape == (1, 3, 3, 13, 13) and out.dtype == torch.float32
    run = Launch([(a_dev, good, color)], 13, 13, _lib.F32, "BTCHW", 1)
    assert torch.equal(out.reshape(-1), run.buf[PAD:PAD + run.n])                                  # the same two launches
    for c in (NONE, rec((), shift=SHIFT), rec((0, 2))):           # no contrast anywhere: one launch, frame means unread
        ref = ar.sample(a_np, good, c, 13, 13, ar.MEAN, ar.STD, ar.GRAY_BGR, True)[0]
        got = call(colors=[c])[0].permute(1, 0, 2, 3).double().cpu().numpy()
        assert ar.ratio(got, ref, ar.bound(good, c, 13, 13, ar.MEAN, ar.STD)) <= 1.0
    assert call(dtype=torch.bfloat16).dtype == torch.bfloat16
    for bad in (dict(good, sh=13), dict(good, sy0=-1), dict(good, rh=0), dict(good, oy0=18)):
        with pytest.raises(ValueError):
            call(params=[bad])
    for bad in (rec((0, 0, 1)), rec((0, 3)), dict(color, alpha=[1.0, float("nan"), 1.0]), dict(color, shift=[0.0, float("inf"), 0.0]),
                dict(op=[0, 1, 2, 0], alpha=[1.0] * 4, shift=[0.0] * 3)):
        with pytest.raises(ValueError):
            call(colors=[bad])
    with pytest.raises(ValueError):
        call(clips=[a_dev.permute(0, 2, 1, 3)])                   # pixels not dense
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(clips=[a_dev.cpu()])


@pytest.mark.parametrize("flip", [0, 1])
def test_zero_op_record_agrees_with_focus_clip_sample(sources, flip):
    """The same taps, another order of operations behind them (x/255 then (x - mean)/std as one fma each, against one fma on
    the byte value): each side is inside its own bound, so the two differ by at most the sum."""
    a_np, a_dev = sources["a"]
    p = dict(sy0=2, sx0=3, sh=17, sw=22, rh=23, rw=29, oy0=5, ox0=9, flip=flip)
    for reverse in (False, True):
        plain = ops.clip_sample([a_dev], [p], 13, 13, ar.MEAN, ar.STD, reverse)
        color = ops.clip_sample_color([a_dev], [p], [NONE], 13, 13, ar.MEAN, ar.STD, ar.GRAY_BGR, reverse)
        tol = clip_ref.bound(p, ar.MEAN, ar.STD) + ar.bound(p, NONE, 13, 13, ar.MEAN, ar.STD)
        r = ar.ratio(color.double().cpu().numpy(), plain.double().cpu().numpy(), tol)
        print("zero ops vs focus_clip_sample, flip %d reverse %d: difference / bound %.3f" % (flip, reverse, r))
        assert r <= 1.0


# ---- the sampler above the kernels --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def z():
    return ar.fixture()


def orvit_for(T, O=2):
    g = np.random.RandomState(11)
    xy = g.uniform(0, 0.5, (T, O, 2))
    ob = np.concatenate([xy, xy + g.uniform(0.1, 0.45, (T, O, 2))], -1)
    ob[1, 1] = 0.0                                                # an absent object
    return ob


@pytest.mark.parametrize("tag", list(ar.CASES))
def test_sample_ava_clips_end_to_end(z, tag):
    cid, split, S, ava = ar.CASES[tag]
    clip, p, color, _, _ = ar.case_plan(z, tag)
    np.random.seed(int(z[tag + ".seed"]))
    inputs, meta = ds.sample_ava_clips(ar.case_cfg(tag), [torch.from_numpy(clip).cuda()], [z["boxes_" + cid]], split, orvit_boxes=[orvit_for(3)])
    assert np.random.uniform() == float(z[tag + ".next"])          # the planner inside, draw for draw
    assert inputs.is_cuda and inputs.dtype == torch.float32 and inputs.shape == (1, 3, 3, S, S)
    got = inputs[0].double().cpu().numpy()
    ref = ar.sample(clip, p, color, S, S, ar.MEAN, ar.STD, ar.GRAY_BGR, not ava.get("BGR", False))[0]
    tol, tol_any = ar.bound(p, color, S, S, ar.MEAN, ar.STD), ar.bound(p, color, S, S, ar.MEAN, ar.STD, any_order=True)
    r, r_rec = ar.ratio(got, ref, tol), ar.ratio(got, z[tag + ".frames"].astype(np.float64), tol + tol_any)
    print("%s: kernel vs fp64 / bound %.3f, kernel vs the reference's frames / (both bounds) %.3f" % (tag, r, r_rec))
    assert r <= 1.0 and r_rec <= 1.0
    n = z["boxes_" + cid].shape[0]
    assert meta["boxes"].dtype == torch.float32 and meta["boxes"].shape == (n, 5) and not meta["boxes"][:, 0].any()
    assert torch.equal(meta["boxes"][:, 1:], torch.from_numpy(z[tag + ".boxes"].astype(np.float32)))
    assert torch.equal(meta["ori_boxes"][:, 1:], torch.from_numpy(z["boxes_" + cid].astype(np.float32))) and meta["ori_boxes"].shape == (n, 5)
    ob = meta["orvit_bboxes"]
    assert ob.shape == (1, 3, 2, 4) and ob.dtype == torch.float32 and not ob[0, 1, 1].any() and float(ob.max()) <= 1.0


def test_sample_ava_clips_batch_of_two_sizes_rgb_source_and_bf16(z):
    cfg = ar.case_cfg("order012")
    rev = not cfg.AVA.BGR
    clips = [z["clip_a"], z["clip_b"]]
    boxes = [z["boxes_a"], z["boxes_b"]]
    np.random.seed(77)
    plans = [ds.ava_plan(cfg, c.shape[1], c.shape[2], b.copy(), "train") for c, b in zip(clips, boxes)]
    np.random.seed(77)
    inputs, meta = ds.sample_ava_clips(cfg, [torch.from_numpy(c).cuda() for c in clips], boxes, "train")
    assert inputs.shape == (2, 3, 3, 13, 13) and "orvit_bboxes" not in meta
    assert meta["boxes"][:, 0].tolist() == [0.0] * 4 + [1.0] * 3 and meta["ori_boxes"][:, 0].tolist() == [0.0] * 4 + [1.0] * 3
    refs = []
    for b, (clip, (p, color, bx)) in enumerate(zip(clips, plans)):
        ref = ar.sample(clip, p, color, 13, 13, ar.MEAN, ar.STD, ar.GRAY_BGR, rev)[0]
        refs.append((ref, ar.bound(p, color, 13, 13, ar.MEAN, ar.STD)))
        assert ar.ratio(inputs[b].double().cpu().numpy(), *refs[-1]) <= 1.0
        assert torch.equal(meta["boxes"][meta["boxes"][:, 0] == b][:, 1:], torch.from_numpy(bx.astype(np.float32)))
    # the same clips decoded as RGB: grey weights, PCA shift, mean / std follow the true colours; the output is the same
    np.random.seed(77)
    rgb, _ = ds.sample_ava_clips(cfg, [torch.from_numpy(np.ascontiguousarray(c[..., ::-1])).cuda() for c in clips], boxes, "train",
                                 source_order="rgb")
    for b in range(2):
        assert ar.ratio(rgb[b].double().cpu().numpy(), *refs[b]) <= 1.0
    cfg.TRAIN.MIXED_PRECISION = True
    np.random.seed(77)
    half, _ = ds.sample_ava_clips(cfg, [torch.from_numpy(c).cuda() for c in clips], boxes, "train")
    assert half.dtype == torch.bfloat16
    for b, (p, color, _) in enumerate(plans):
        tol = ar.bound(p, color, 13, 13, ar.MEAN, ar.STD, ref=refs[b][0], bf16=True)
        assert ar.ratio(half[b].double().cpu().numpy(), refs[b][0], tol) <= 1.0


def test_test_split_without_centre_crop(z):
    cfg = ar.case_cfg("val")
    cfg.AVA.CENTER_CROP_TEST = False
    a = torch.from_numpy(z["clip_a"]).cuda()
    np.random.seed(1)
    inputs, meta = ds.sample_ava_clips(cfg, [a, a], [z["boxes_a"], z["boxes_a"]], "test")
    assert inputs.shape == (2, 3, 3, 16, 21) and torch.equal(inputs[0], inputs[1])
    assert float(meta["boxes"][:, [1, 3]].max()) <= 20.0 and 14.0 < float(meta["boxes"][:, 4].max()) <= 15.0
    with pytest.raises(ValueError, match="one size"):
        ds.sample_ava_clips(cfg, [a, torch.from_numpy(z["clip_b"]).cuda()], [z["boxes_a"], z["boxes_b"]], "test")


def det_batch(mixed):
    from test_roi_head_ref_cpu import _det_cfg
    cfg = _det_cfg(["TRAIN.MIXED_PRECISION", mixed, "DATA.TRAIN_JITTER_SCALES", [36, 44], "AVA.TRAIN_USE_COLOR_AUGMENTATION", True,
                    "AVA.TRAIN_PCA_JITTER_ONLY", False, "SOLVER.OPTIMIZING_METHOD", "sgd", "SOLVER.BASE_LR", 0.1,
                    "SOLVER.WEIGHT_DECAY", 0.0])
    g = torch.Generator().manual_seed(3)
    clips = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).cuda() for s in ((4, 40, 52, 3), (4, 48, 38, 3))]
    boxes = [np.array([[0.1, 0.1, 0.8, 0.9], [0.3, 0.2, 0.6, 0.7]]), np.array([[0.05, 0.3, 0.9, 0.95]])]
    np.random.seed(5)
    inputs, meta = ds.sample_ava_clips(cfg, clips, boxes, "train")
    assert inputs.shape == (2, 3, 4, 32, 32) and meta["boxes"].shape == (3, 5)
    return cfg, inputs, meta


def test_a_batch_goes_into_the_detection_mvit_in_bf16():
    from focus_amd.slowfast.models import build_model
    cfg, inputs, meta = det_batch(True)
    assert inputs.dtype == torch.bfloat16
    torch.manual_seed(0)
    m = build_model(cfg).eval()
    with torch.no_grad():
        y = m([inputs], {}, bboxes=meta["boxes"])
    assert y.shape == (3, 5) and bool(torch.isfinite(y.float()).all()) and bool(((y > 0) & (y < 1)).all())


def test_one_training_step_with_the_returned_meta():
    from focus_amd.slowfast.models import build_model
    from focus_amd.slowfast.models.losses import get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    from focus_amd.train import train_iter
    cfg, inputs, meta = det_batch(False)
    torch.manual_seed(0)
    m = build_model(cfg).train()
    opt = construct_optimizer(m, cfg)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    labels = (torch.rand(3, 5, generator=torch.Generator().manual_seed(1)) > 0.6).float().cuda()
    w0 = m.head.projection.weight.detach().clone()
    preds, _, loss = train_iter(m, opt, loss_fun, [inputs], labels, {k: v.cuda() for k, v in meta.items()}, cfg)
    assert preds.shape == (3, 5) and np.isfinite(float(loss.detach()))
    assert float((m.head.projection.weight.detach() - w0).abs().max()) > 0
