"""focus_clip_sample by the C ABI with explicit descriptors, and the sampler above it, against the fp64 formula of
tests/clip_ref.py within the bound derived there.  Shapes are the smallest that reach each hazard: 81-byte source rows and a
padded row stride, 13x13 outputs (scalar tail, odd row bases) and 16x8 outputs (16-byte stores), two clips of different size
and flip in one launch, the second-tap clamp on the last source row and column, a >= 2x downscale, a window offset."""
import ctypes
import random

import numpy as np
import pytest
import torch

import clip_ref
from focus_amd import _lib, ops
from focus_amd.slowfast.config.defaults import get_cfg
from focus_amd.slowfast.datasets import device_sampling as ds
from focus_amd.slowfast.datasets import utils as du

pytestmark = pytest.mark.gpu

CANARY = -768.0               # exact in bf16 too
PAD = 64                      # elements on both sides of the output: a multiple of 16 bytes in both dtypes
NULL, SHAPE, DTYPE = -5, -1, -2
TDT = {_lib.F32: torch.float32, _lib.BF16: torch.bfloat16}


@pytest.fixture(scope="module")
def z():
    return clip_ref.fixture()


@pytest.fixture(scope="module")
def sources(z):
    """name -> (numpy [T,H,W,3], device tensor viewing it): clip a dense (81-byte rows), a 2x40x64 clip inside rows padded to
    200 bytes and frames padded by one row."""
    g = torch.Generator().manual_seed(5)
    big = torch.randint(0, 256, (2, 40, 64, 3), generator=g, dtype=torch.uint8)
    buf = torch.full((2, 41, 200), 255, dtype=torch.uint8, device="cuda")
    view = buf[:, :40, :192].unflatten(2, (64, 3))
    view.copy_(big)
    assert view.stride() == (8200, 200, 3, 1)
    a = torch.from_numpy(z["clip_a"]).cuda()
    assert a.stride() == (1620, 81, 3, 1)
    return {"a": (z["clip_a"], a), "big": (big.numpy(), view)}


def items_table(entries):
    """focus_clip_item records written by hand: (device clip, params) -> int64 [n, 9] on the device."""
    rec = np.zeros((len(entries), 9), dtype=np.int64)
    for i, (c, p) in enumerate(entries):
        ints = [c.shape[1], c.shape[2], p["sy0"], p["sx0"], p["sh"], p["sw"], p["rh"], p["rw"], p["oy0"], p["ox0"], p["flip"], 0]
        rec[i, :3] = c.data_ptr(), c.stride(1), c.stride(0)
        rec[i, 3:] = [ints[2 * k] | (ints[2 * k + 1] << 32) for k in range(6)]
    return torch.from_numpy(rec).cuda()


def f3(v):
    arr = (ctypes.c_float * 3)(*v)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def launch(entries, out_h, out_w, dtype, layout, reverse, mean, std, shift=0):
    """One call of the C entry point into a canary-framed buffer -> (status, float64 [B,3,T,h,w], the framed buffer).
    shift: extra elements before the output (a base that is not 16-byte aligned)."""
    B, T = len(entries), entries[0][0].shape[0]
    plane = out_h * out_w
    n = B * 3 * T * plane
    buf = torch.full((PAD + shift + n + PAD,), CANARY, dtype=TDT[dtype], device="cuda")
    out = buf[PAD + shift:PAD + shift + n]
    sc, st = (T * plane, plane) if layout == "BCTHW" else (plane, 3 * plane)
    items = items_table(entries)
    keep_m, m = f3(mean)
    keep_s, s = f3(std)
    status = _lib.lib().focus_clip_sample(ctypes.c_void_p(items.data_ptr()), B, T, out_h, out_w, ctypes.c_void_p(out.data_ptr()),
                                          3 * T * plane, sc, st, m, s, int(reverse), dtype,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    res = out.double().cpu().numpy()
    res = res.reshape(B, 3, T, out_h, out_w) if layout == "BCTHW" else res.reshape(B, T, 3, out_h, out_w).transpose(0, 2, 1, 3, 4)
    return status, res, buf


def canaries_intact(buf, n_out, shift=0):
    head, tail = buf[:PAD + shift].float().cpu(), buf[PAD + shift + n_out:].float().cpu()
    return bool((head == CANARY).all()) and bool((tail == CANARY).all()) and tail.numel() == PAD


def check(entries_np, res, out_h, out_w, dtype, reverse, mean, std, coords=True, label=""):
    worst = 0.0
    for b, (src, p) in enumerate(entries_np):
        ref = clip_ref.sample(src, p, out_h, out_w, mean, std, reverse)
        tol = clip_ref.bound(p, mean, std, ref=ref, bf16=dtype == _lib.BF16, coords=coords)
        worst = max(worst, clip_ref.ratio(res[b], ref, tol))
    print("%s error / bound %.3f" % (label, worst))
    assert worst <= 1.0
    return worst


def pair_params(out_h, out_w):
    """Clip a: a rectangle ending on the last source row and column, upscaled 2.4x, the window at the far end of the resized
    image (second-tap clamp), mirrored.  The big clip: the whole frame downscaled 2.2x, an interior window, not mirrored."""
    pa = dict(sy0=8, sx0=14, sh=12, sw=13, rh=30, rw=31, oy0=30 - out_h, ox0=31 - out_w, flip=1)
    pb = dict(sy0=0, sx0=0, sh=40, sw=64, rh=18, rw=29, oy0=17 - out_h, ox0=7, flip=0)
    return pa, pb


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("layout", ["BCTHW", "BTCHW"])
@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
@pytest.mark.parametrize("out_hw", [(13, 13), (16, 8)])
def test_two_clips_one_launch(sources, out_hw, dtype, layout, reverse):
    out_h, out_w = out_hw
    pa, pb = pair_params(out_h, out_w)
    # the launch takes one T: the first two frames of clip a beside the two of the big clip
    a_np, a_dev = sources["a"][0][:2], sources["a"][1][:2]
    b_np, b_dev = sources["big"]
    status, res, buf = launch([(a_dev, pa), (b_dev, pb)], out_h, out_w, dtype, layout, reverse, clip_ref.MEAN, clip_ref.STD)
    assert status == 0
    assert canaries_intact(buf, res.size)
    check([(a_np, pa), (b_np, pb)], res, out_h, out_w, dtype, reverse, clip_ref.MEAN, clip_ref.STD,
          label="%dx%d %s %s reverse %d:" % (out_h, out_w, TDT[dtype], layout, reverse))


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
def test_vector_shape_on_a_base_that_is_not_16_byte_aligned(sources, dtype):
    pa, _ = pair_params(16, 8)
    a_np, a_dev = sources["a"]
    status, res, buf = launch([(a_dev, pa)], 16, 8, dtype, "BCTHW", 1, clip_ref.MEAN, clip_ref.STD, shift=3)
    assert status == 0 and canaries_intact(buf, res.size, shift=3)
    check([(a_np, pa)], res, 16, 8, dtype, 1, clip_ref.MEAN, clip_ref.STD, label="16x8 shifted %s:" % TDT[dtype])


@pytest.mark.parametrize("flip", [0, 1])
def test_scale_one_is_tensor_normalize(sources, flip):
    """rh = sh, rw = sw: every source coordinate is a whole number, the bilinear weights are 0 and 1, and what is left is the
    normalisation: equal to tensor_normalize within the arithmetic term alone."""
    a_np, a_dev = sources["a"]
    p = dict(sy0=3, sx0=5, sh=14, sw=20, rh=14, rw=20, oy0=1, ox0=4, flip=flip)
    status, res, buf = launch([(a_dev, p)], 13, 13, _lib.F32, "BCTHW", 0, clip_ref.MEAN, clip_ref.STD)
    assert status == 0 and canaries_intact(buf, res.size)
    check([(a_np, p)], res, 13, 13, _lib.F32, 0, clip_ref.MEAN, clip_ref.STD, coords=False, label="scale 1 flip %d:" % flip)
    norm = du.tensor_normalize(torch.from_numpy(a_np), clip_ref.MEAN, clip_ref.STD)[:, 4:17, 9:22].permute(3, 0, 1, 2)
    norm = (norm.flip(-1) if flip else norm).double().numpy()
    tol = 2 * clip_ref.bound(p, clip_ref.MEAN, clip_ref.STD, coords=False)          # both sides carry the arithmetic term
    print("scale 1 vs tensor_normalize: error / bound %.3f" % clip_ref.ratio(res[0], norm, tol))
    assert clip_ref.ratio(res[0], norm, tol) <= 1.0


def test_two_calls_give_the_same_bits(sources):
    pa, pb = pair_params(13, 13)
    entries = [(sources["a"][1][:2], pa), (sources["big"][1], pb)]
    outs = [launch(entries, 13, 13, _lib.BF16, "BCTHW", 1, clip_ref.MEAN, clip_ref.STD)[2] for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_refusals_write_nothing(sources):
    lib = _lib.lib()
    a_dev = sources["a"][1]
    p = pair_params(13, 13)[0]
    items = items_table([(a_dev, p)])
    buf = torch.full((4096,), CANARY, device="cuda")
    ip, op = ctypes.c_void_p(items.data_ptr()), ctypes.c_void_p(buf.data_ptr())
    (km, m), (ks, s) = f3(clip_ref.MEAN), f3(clip_ref.STD)
    call = lambda it, n, T, h, w, o, mm, ss, dt: lib.focus_clip_sample(it, n, T, h, w, o, 3 * T * h * w, T * h * w, h * w, mm, ss, 0,
                                                                        dt, None)
    assert call(None, 1, 3, 13, 13, op, m, s, _lib.F32) == NULL
    assert call(ip, 1, 3, 13, 13, None, m, s, _lib.F32) == NULL
    assert call(ip, 1, 3, 13, 13, op, None, s, _lib.F32) == NULL
    assert call(ip, 1, 3, 13, 13, op, m, None, _lib.F32) == NULL
    assert call(None, 0, 3, 0, 13, op, m, s, 7) == NULL                     # NULL is judged first
    assert call(ip, 0, 3, 13, 13, op, m, s, _lib.F32) == 0                  # nothing to do: no launch
    assert call(ip, -1, 3, 0, 13, op, m, s, 7) == 0 and call(ip, 1, 0, 13, 13, op, m, s, _lib.F32) == 0
    assert call(ip, 1, 3, 0, 13, op, m, s, _lib.F32) == SHAPE and call(ip, 1, 3, 13, -2, op, m, s, _lib.F32) == SHAPE
    assert call(ip, 1, 3, 0, 13, op, m, s, 7) == SHAPE                      # the shape is judged before the dtype
    assert call(ip, 1, 3, 13, 13, op, m, s, _lib.FP8_E4M3) == DTYPE and call(ip, 1, 3, 13, 13, op, m, s, -1) == DTYPE
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    assert call(ip, 1, 3, 13, 13, op, m, s, _lib.F32) == 0                  # and the same arguments, accepted, do write
    torch.cuda.synchronize()
    assert bool((buf[:3 * 3 * 169] != CANARY).all()) and bool((buf[3 * 3 * 169:] == CANARY).all())


def test_wrapper_validates_what_the_kernel_cannot(sources):
    a_np, a_dev = sources["a"]
    good = dict(sy0=8, sx0=14, sh=12, sw=13, rh=30, rw=31, oy0=17, ox0=18, flip=1)
    out = ops.clip_sample([a_dev], [good], 13, 13, clip_ref.MEAN, clip_ref.STD, True, torch.float32, "BTCHW")
    assert out.shape == (1, 3, 3, 13, 13)
    ref = clip_ref.sample(a_np, good, 13, 13, clip_ref.MEAN, clip_ref.STD, True)
    assert clip_ref.ratio(out[0].permute(1, 0, 2, 3).double().cpu().numpy(), ref, clip_ref.bound(good, clip_ref.MEAN, clip_ref.STD)) <= 1.0
    for bad in (dict(good, sh=13), dict(good, sx0=15), dict(good, sy0=-1), dict(good, sw=0), dict(good, rh=0),
                dict(good, oy0=18), dict(good, ox0=-1)):
        with pytest.raises(ValueError):
            ops.clip_sample([a_dev], [bad], 13, 13, clip_ref.MEAN, clip_ref.STD)
    with pytest.raises(ValueError):
        ops.clip_sample([a_dev.permute(0, 2, 1, 3)], [good], 13, 13, clip_ref.MEAN, clip_ref.STD)      # pixels not dense
    with pytest.raises(ValueError):
        ops.clip_sample([a_dev, a_dev[:2]], [good, good], 13, 13, clip_ref.MEAN, clip_ref.STD)         # two T in one launch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clip_sample([a_dev.cpu()], [good], 13, 13, clip_ref.MEAN, clip_ref.STD)


def sampler_cfg(model="Motionformer", mixed=False):
    cfg = get_cfg()
    cfg.DATA.MEAN, cfg.DATA.STD, cfg.DATA.REVERSE_INPUT_CHANNEL = list(clip_ref.MEAN), list(clip_ref.STD), True
    cfg.MODEL.MODEL_NAME = model
    cfg.TRAIN.MIXED_PRECISION = mixed
    return cfg


def run_sampler(z, tag, cfg):
    cid, kw = clip_ref.CASES[tag]
    seed = int(z[tag + ".seed"])
    random.seed(seed)
    np.random.seed(seed)
    p, _ = ds.sampling_params(z["clip_" + cid].shape[1], z["clip_" + cid].shape[2], random_horizontal_flip=True, **kw)
    random.seed(seed)
    np.random.seed(seed)
    inputs, ob = ds.sample_clips(cfg, [torch.from_numpy(z["clip_" + cid]).cuda()], [z["boxes_" + cid]], random_horizontal_flip=True, **kw)
    return z["clip_" + cid], p, inputs, ob


@pytest.mark.parametrize("tag", list(clip_ref.CASES))
def test_sample_clips_end_to_end(z, tag):
    clip, p, inputs, ob = run_sampler(z, tag, sampler_cfg())
    S = p["out_h"]
    assert inputs.is_cuda and inputs.dtype == torch.float32 and inputs.shape == (1, 3, clip.shape[0], S, S)
    ref = clip_ref.sample(clip, p, S, S, clip_ref.MEAN, clip_ref.STD, True)
    tol = clip_ref.bound(p, clip_ref.MEAN, clip_ref.STD)
    got = inputs[0].double().cpu().numpy()
    print("%s: kernel / bound %.3f, reference fp32 / bound %.3f" % (tag, clip_ref.ratio(got, ref, tol),
                                                                     clip_ref.ratio(z[tag + ".frames"], ref, tol)))
    assert clip_ref.ratio(got, ref, tol) <= 1.0
    assert not ob.is_cuda and ob.shape == (1,) + z[tag + ".orvit_bboxes"].shape
    assert torch.equal(ob[0], torch.from_numpy(z[tag + ".orvit_bboxes"]))


def test_sample_clips_for_steve_in_bf16(z):
    """MODEL_NAME STEVE: [B,T,C,H,W] in [0,1] without reversal; TRAIN.MIXED_PRECISION: bf16."""
    clip, p, inputs, ob = run_sampler(z, "rrc_flip", sampler_cfg("STEVE", True))
    assert inputs.dtype == torch.bfloat16 and inputs.shape == (1, clip.shape[0], 3, 13, 13)
    ref = clip_ref.sample(clip, p, 13, 13, [0.0] * 3, [1.0] * 3, False)
    tol = clip_ref.bound(p, [0.0] * 3, [1.0] * 3, ref=ref, bf16=True)
    assert clip_ref.ratio(inputs[0].permute(1, 0, 2, 3).double().cpu().numpy(), ref, tol) <= 1.0
    assert float(inputs.min()) >= 0.0 and float(inputs.max()) <= 1.0
    assert torch.equal(ob[0], torch.from_numpy(z["rrc_flip.orvit_bboxes"]))
