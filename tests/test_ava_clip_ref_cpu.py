"""Host side of the AVA clip front end, no GPU: the mirror colour functions and the planner of `sample_ava_clips` against a
fixture written by the reference's own transform.py (tests/make_ava_clip_golden.py) -- frames and boxes bit for bit, the draws
counted by the recorded follow-up draw --, the single-pass formula the kernels implement (tests/ava_clip_ref.py) against the
same fixture inside the derived bound, every named wrong variant outside it, the refusals of ops.clip_sample_color that need
no device, and the config defaults."""
import numpy as np
import pytest
import torch

import ava_clip_ref as ar
from focus_amd import ops
from focus_amd.slowfast.config.defaults import get_cfg
from focus_amd.slowfast.datasets import device_sampling as ds
from focus_amd.slowfast.datasets import transform

TAGS = list(ar.CASES)


@pytest.fixture(scope="module")
def z():
    return ar.fixture()


def mirror(z, tag):
    """ava_dataset.py:268-365 on CPU tensors through the mirror functions of datasets/transform.py -> ([3,T,S,S], boxes, the
    draw that follows)."""
    cid, split, crop, _ = ar.CASES[tag]
    cfg = ar.case_cfg(tag)
    np.random.seed(int(z[tag + ".seed"]))
    imgs = torch.from_numpy(z["clip_" + cid]).permute(0, 3, 1, 2).float() / 255.0
    boxes = z["boxes_" + cid].copy()
    h, w = imgs.shape[2:]
    boxes[:, [0, 2]] *= w
    boxes[:, [1, 3]] *= h
    boxes = transform.clip_boxes_to_image(boxes, h, w)
    if split == "train":
        imgs, boxes = transform.random_short_side_scale_jitter(imgs, *ar.JITTER[crop], boxes=boxes)
        imgs, boxes = transform.random_crop(imgs, crop, boxes=boxes)
        imgs, boxes = transform.horizontal_flip(0.5, imgs, boxes=boxes)
    else:
        imgs, boxes = transform.random_short_side_scale_jitter(imgs, crop, crop, boxes=boxes)
        imgs, boxes = transform.uniform_crop(imgs, crop, 1, boxes=boxes)
        if cfg.AVA.TEST_FORCE_FLIP:
            imgs, boxes = transform.horizontal_flip(1, imgs, boxes=boxes)
    if split == "train" and cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION:
        if not cfg.AVA.TRAIN_PCA_JITTER_ONLY:
            imgs = transform.color_jitter(imgs, 0.4, 0.4, 0.4)
        imgs = transform.lighting_jitter(imgs, 0.1, np.array(ar.EIGVAL).astype(np.float32), np.array(ar.EIGVEC).astype(np.float32))
    imgs = transform.color_normalization(imgs, np.array(ar.MEAN, dtype=np.float32), np.array(ar.STD, dtype=np.float32))
    if not cfg.AVA.BGR:
        imgs = imgs[:, [2, 1, 0], ...]
    return imgs.permute(1, 0, 2, 3), transform.clip_boxes_to_image(boxes, crop, crop), np.random.uniform()


def test_fixture_holds_what_the_cases_need(z):
    assert z["clip_a"].shape == (3, 20, 27, 3) and z["clip_b"].shape == (3, 24, 17, 3) and z["clip_a"].dtype == np.uint8
    assert z["boxes_a"].shape == (4, 4) and z["boxes_b"].shape == (3, 4) and z["boxes_a"].min() < 0 and z["boxes_a"].max() > 1
    plans = {tag: ar.case_plan(z, tag) for tag in TAGS}
    assert [tuple(plans["order%d%d%d" % o][2]["op"]) for o in ar.ORDERS] == ar.ORDERS          # all six drawn orders
    flips = [plans["order%d%d%d" % o][1]["flip"] for o in ar.ORDERS]
    assert 0 in flips and 1 in flips
    assert plans["pca_only"][2]["op"] == [] and max(abs(s) for s in plans["pca_only"][2]["shift"]) > 0
    assert plans["no_color"][2] == dict(op=[], alpha=[], shift=[0.0, 0.0, 0.0])
    assert plans["val"][1]["flip"] == 0 and plans["val_flip"][1]["flip"] == 1
    assert {z[t + ".frames"].shape[-1] for t in TAGS} == {13, 16}
    means = z["clip_a"].reshape(3, -1).mean(1)                    # frames at unlike brightness: per-frame vs clip-wide mean
    assert means[0] > 1.5 * means[1] > 2.5 * means[2]


@pytest.mark.parametrize("tag", TAGS)
def test_mirror_functions_give_the_references_frames_and_boxes(z, tag):
    frames, boxes, nxt = mirror(z, tag)
    assert torch.equal(frames, torch.from_numpy(z[tag + ".frames"]))
    assert boxes.dtype == z[tag + ".boxes"].dtype and np.array_equal(boxes, z[tag + ".boxes"])
    assert nxt == float(z[tag + ".next"])


@pytest.mark.parametrize("tag", TAGS)
def test_planner_draws_and_boxes_are_the_references(z, tag):
    clip, p, color, boxes, nxt = ar.case_plan(z, tag)
    S = ar.CASES[tag][2]
    assert nxt == float(z[tag + ".next"])                          # draw for draw
    assert np.array_equal(boxes, z[tag + ".boxes"])
    assert (p["out_h"], p["out_w"]) == (S, S)
    assert 0 <= p["oy0"] and p["oy0"] + S <= p["rh"] and 0 <= p["ox0"] and p["ox0"] + S <= p["rw"]
    assert boxes.min() >= 0 and boxes.max() <= S - 1


def test_color_plan_consumes_the_draws_of_the_functions():
    x = torch.rand(2, 3, 5, 6)
    ev, evec = np.array(ar.EIGVAL).astype(np.float32), np.array(ar.EIGVEC).astype(np.float32)
    for args in ((0.4, 0.4, 0.4, 0.1), (0, 0, 0, 0.1), (0.4, 0, 0.3, 0), (0, 0.2, 0, 0.1)):
        np.random.seed(7)
        y = transform.lighting_jitter(transform.color_jitter(x, *args[:3]), args[3], ev, evec)
        after = np.random.uniform()
        np.random.seed(7)
        plan = transform.color_plan(*args, ev, evec)
        assert after == np.random.uniform()
        assert len(plan["op"]) == sum(v != 0 for v in args[:3]) and len(set(plan["op"])) == len(plan["op"])
        # the plan through the single-pass formula is the functions' result (BGR positions: shift as planned)
        ref = ar.color_stage(x.permute(0, 2, 3, 1).double().numpy(), plan, ar.GRAY_BGR, np.float64)[0]
        assert np.abs(y.permute(0, 2, 3, 1).double().numpy() - ref).max() < 1e-5


def test_the_test_split_without_centre_crop_keeps_the_resized_frame(z):
    cfg = ar.case_cfg("val")
    cfg.AVA.CENTER_CROP_TEST = False
    np.random.seed(3)
    p, color, boxes = ds.ava_plan(cfg, 20, 27, z["boxes_a"].copy(), "test")
    assert (p["out_h"], p["out_w"], p["rh"], p["rw"], p["oy0"], p["ox0"]) == (16, 21, 16, 21, 0, 0) and color["op"] == []
    np.random.seed(3)
    _, want = transform.random_short_side_scale_jitter(torch.zeros(1, 3, 20, 27), 16, 16, boxes=transform.clip_boxes_to_image(
        z["boxes_a"] * np.array([27, 20, 27, 20.0]), 20, 27))
    assert np.array_equal(boxes, transform.clip_boxes_to_image(want, 16, 21))          # clipped to the real output size
    cfg.AVA.CENTER_CROP_TEST = True
    assert ds.ava_plan(cfg, 20, 27, z["boxes_a"].copy(), "test")[0]["out_w"] == 16
    with pytest.raises(NotImplementedError):
        ds.ava_plan(cfg, 20, 27, z["boxes_a"].copy(), "trainval")


def case_refs(z, tag):
    clip, p, color, _, _ = ar.case_plan(z, tag)
    S, rev = p["out_h"], not ar.CASES[tag][3].get("BGR", False)
    args = (clip, p, color, S, S, ar.MEAN, ar.STD, ar.GRAY_BGR, rev)
    return args, ar.sample(*args)[0], ar.bound(p, color, S, S, ar.MEAN, ar.STD), ar.bound(p, color, S, S, ar.MEAN, ar.STD, any_order=True)


@pytest.mark.parametrize("tag", TAGS)
def test_formula_and_its_fp32_twin_are_inside_the_bound(z, tag):
    args, ref, tol, tol_any = case_refs(z, tag)
    r_fix = ar.ratio(z[tag + ".frames"], ref, tol_any)
    twin, means = ar.sample(*args, dtype=np.float32)
    r_twin = ar.ratio(twin, ref, tol)
    print("%s: bound %.3e (any order %.3e), reference fp32 / bound %.3f, fp32 twin / bound %.3f" % (tag, tol, tol_any, r_fix, r_twin))
    assert twin.dtype == np.float32 and r_fix <= 1.0 and r_twin <= 1.0
    color, p = args[2], args[1]
    if ar.CONTRAST in color["op"]:
        r_mean = ar.ratio(means, ar.sample(*args)[1], ar.mean_bound(p, color, p["out_h"], p["out_w"]))
        print("%s: frame mean twin / bound %.3f" % (tag, r_mean))
        assert r_mean <= 1.0
    else:
        assert not means.any()


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_every_wrong_variant_is_outside_the_bound(z, mutant):
    worst = {}
    for tag in TAGS:
        args, ref, tol, _ = case_refs(z, tag)
        worst[tag] = ar.ratio(ar.sample(*args, dtype=np.float32, mutant=mutant)[0], ref, tol)
    print("%s: error / bound " % mutant + " ".join("%s %.3g" % kv for kv in worst.items()))
    assert max(worst.values()) > 1.0
    if mutant in ar.MUTANT_CASE:
        assert worst[ar.MUTANT_CASE[mutant]] > 1.0


def test_moving_an_op_with_its_alpha_is_no_mutant(z):
    """The three ops commute in exact arithmetic (sum(gray_w) = 1): the drawn order matters through the draws alone."""
    for tag in ("order%d%d%d" % o for o in ar.ORDERS):
        args, ref, tol, _ = case_refs(z, tag)
        assert ar.ratio(ar.sample(*args, mutant="reordered")[0], ref, tol) <= 1.0


def test_bound_terms():
    p = dict(sh=20, sw=27)
    none = dict(op=[], alpha=[], shift=[0.0] * 3)
    base = ar.bound(p, none, 13, 13, ar.MEAN, ar.STD)
    assert base == pytest.approx((9 + 3 * 49 + 1 + 4 * 1.35) * ar.U / 0.2)
    assert ar.bound(p, none, 13, 13, ar.MEAN, ar.STD, coords=False) < base
    con = dict(op=[1], alpha=[1.3], shift=[0.0] * 3)
    assert ar.mean_depth(13, 13) == 8 + 6 + 4 + 1 and ar.mean_depth(40, 56) == 8 + 6 + 4 + 2 and ar.mean_depth(13, 13, True) == 506
    assert ar.bound(p, con, 40, 56, ar.MEAN, ar.STD) > ar.bound(p, con, 13, 13, ar.MEAN, ar.STD) > 1.6 * base      # gain 1.6
    assert ar.mean_bound(p, con, 13, 13) == pytest.approx((9 + 3 * 49 + 8 + 19 + 1) * ar.U)
    ref = np.full((2, 2), 3.0)
    assert np.allclose(ar.bound(p, none, 13, 13, ar.MEAN, ar.STD, ref=ref, bf16=True), base + 3.0 / 256)


def test_clip_sample_color_refuses_without_a_device():
    good = dict(op=[2, 0, 1], alpha=[1.1, 0.9, 1.2], shift=[0.01, -0.02, 0.0])
    rec = ops.clip_colors([good, dict(op=[], alpha=[], shift=[0, 0, 0])], 2)
    assert rec.shape == (2, 10) and rec.dtype == np.int32 and rec.nbytes == 80
    assert rec[0, :4].tolist() == [3, 2, 0, 1] and rec[1].tolist() == [0] * 10
    assert rec.view(np.float32)[0, 4:].tolist() == [np.float32(v) for v in (1.1, 0.9, 1.2, 0.01, -0.02, 0.0)]
    for bad in (dict(good, op=[0, 1, 2, 0], alpha=[1, 1, 1, 1]), dict(good, op=[0, 0, 1]), dict(good, op=[0, 1, 3]),
                dict(good, op=[0, -1, 1]), dict(good, alpha=[1.0, 1.0]), dict(good, alpha=[1.0, float("nan"), 1.0]),
                dict(good, alpha=[1.0, float("inf"), 1.0]), dict(good, shift=[0.0, float("inf"), 0.0]), dict(good, shift=[0.0, 0.0])):
        with pytest.raises(ValueError):
            ops.clip_colors([bad], 1)
    with pytest.raises(ValueError):
        ops.clip_colors([good], 2)
    clip = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    p = dict(sy0=0, sx0=0, sh=8, sw=8, rh=8, rw=8, oy0=0, ox0=0, flip=0)
    call = lambda **kw: ops.clip_sample_color(**dict(dict(clips=[clip], params=[p], colors=[good], out_h=8, out_w=8, mean=ar.MEAN,
                                                          std=ar.STD, gray_w=ar.GRAY_BGR), **kw))
    for kw in (dict(layout="BHWC"), dict(out_h=0), dict(std=[1.0, 0.0, 1.0]), dict(mean=[0.0, 0.0]), dict(gray_w=[0.5, 0.5]),
               dict(gray_w=[0.1, float("nan"), 0.2]), dict(colors=[]), dict(colors=[dict(good, op=[1, 1, 0])]), dict(params=[])):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        call(dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ds.sample_ava_clips(ar.case_cfg("val"), [clip], [np.array([[0.1, 0.1, 0.6, 0.7]])], "val")
    with pytest.raises(ValueError):
        ds.sample_ava_clips(ar.case_cfg("val"), [clip], [np.zeros((1, 4))], "val", source_order="gbr")


def test_config_defaults_are_the_references():
    cfg = get_cfg()
    a = cfg.AVA
    assert (a.BGR, a.TRAIN_USE_COLOR_AUGMENTATION, a.TRAIN_PCA_JITTER_ONLY, a.TEST_FORCE_FLIP, a.CENTER_CROP_TEST,
            a.IMG_PROC_BACKEND) == (False, False, True, False, True, "cv2")
    assert cfg.DATA.TRAIN_PCA_EIGVAL == ar.EIGVAL and cfg.DATA.TRAIN_PCA_EIGVEC == ar.EIGVEC


def test_abi_declares_the_colour_entry_points():
    from focus_amd import _lib
    decl = _lib.parse_header()
    import ctypes
    assert decl["focus_clip_color_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    assert len(decl["focus_clip_gray_mean"][1]) == 11 and decl["focus_clip_gray_mean"][1][6:9] == [ctypes.c_void_p] * 3
    assert len(decl["focus_clip_sample_color"][1]) == 17 and decl["focus_clip_sample_color"][1][13] == ctypes.c_void_p
    lib = _lib.lib()
    assert lib.focus_clip_color_workspace_bytes(2, 3, 13, 13) == 2 * 3 * 2 * 4           # one counter, one partial per frame
    assert lib.focus_clip_color_workspace_bytes(2, 3, 40, 56) == 2 * 3 * 3 * 4           # two blocks per frame
    assert lib.focus_clip_color_workspace_bytes(8, 16, 224, 224) == 8 * 16 * 26 * 4
    assert lib.focus_clip_color_workspace_bytes(0, 3, 13, 13) == 0 == lib.focus_clip_color_workspace_bytes(2, 3, 0, 13)
