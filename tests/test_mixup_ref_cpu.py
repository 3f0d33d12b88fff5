"""CPU-side checks of the mixup path: the twin of tests/mixup_ref.py against the reference's recorded outputs
(tests/golden/mixup.npz) and against ATen's bf16 operations, the mirror MixUp class on CPU tensors, the argument checks of
the four entry points of csrc/mixup.hip (no launch happens, so no GPU is needed), and the loss lookup."""
import ctypes

import numpy as np
import pytest
import torch

import mixup_ref
from focus_amd.slowfast.config.defaults import get_cfg

NULL, SHAPE, DTYPE = -5, -1, -2


@pytest.fixture(scope="module")
def z():
    return mixup_ref.fixture()


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def case_inputs(z, tag):
    B = mixup_ref.CASES[tag][0]
    x = torch.from_numpy(z["x"][:B].copy())
    if tag == "ek_dict":
        return x, {k: torch.from_numpy(z["ek." + k][:B].copy()) for k in ("verb", "noun")}
    return x, torch.from_numpy(z["labels"][:B].copy())


def case_targets(z, tag):
    """{key or None: (labels numpy, num_classes, recorded target numpy)}"""
    B = mixup_ref.CASES[tag][0]
    if tag == "ek_dict":
        return {k: (z["ek." + k][:B], mixup_ref.EK_CLASSES[k], z[tag + ".target." + k]) for k in ("verb", "noun")}
    return {None: (z["labels"][:B], mixup_ref.NUM_CLASSES, z[tag + ".target"])}


def test_fixture_reaches_every_case(z):
    """The recorded draws are the branches the cases are named after."""
    box = {t: tuple(int(v) for v in z[t + ".box"]) for t in mixup_ref.CASES}
    for t in ("blend_even", "blend_odd", "mixup_only", "ek_dict"):
        assert int(z[t + ".cutmix"]) == 0 and 0.0 < float(z[t + ".lam"]) < 1.0 and float(z[t + ".lam"]) != 0.5
    assert mixup_ref.CASES["blend_odd"][0] % 2 == 1 and mixup_ref.CASES["blend_even"][0] % 2 == 0
    yl, yh, xl, xh = box["cutmix_interior"]
    assert int(z["cutmix_interior.cutmix"]) == 1 and 0 < yl < yh < mixup_ref.H and 0 < xl < xh < mixup_ref.W
    yl, yh, xl, xh = box["cutmix_clipped"]
    assert yl < yh and xl < xh and (yl == 0 or xl == 0 or yh == mixup_ref.H or xh == mixup_ref.W)
    assert float(z["cutmix_clipped.lam"]) != float(z["cutmix_clipped.lam_drawn"])
    yl, yh, xl, xh = box["cutmix_empty"]
    assert int(z["cutmix_empty.cutmix"]) == 1 and (yh - yl) * (xh - xl) == 0 and float(z["cutmix_empty.lam"]) == 1.0
    assert float(z["cutmix_empty.lam_drawn"]) != 1.0
    assert float(z["no_mix.lam"]) == 1.0 and np.array_equal(z["no_mix.clip"], z["x"][:2])
    assert int(z["cutmix_only.cutmix"]) == 1


@pytest.mark.parametrize("tag", list(mixup_ref.CASES))
def test_twin_equals_the_reference_bit_for_bit(z, tag):
    x, _ = case_inputs(z, tag)
    lam = float(z[tag + ".lam"])
    if int(z[tag + ".cutmix"]):
        got = mixup_ref.paste(x, *[int(v) for v in z[tag + ".box"]])
    elif lam == 1.0:
        got = x
    else:
        got = mixup_ref.blend(x, lam)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), z[tag + ".clip"])
    smoothing = mixup_ref.case_args(tag).get("label_smoothing", 0.1)
    for labels, V, want in case_targets(z, tag).values():
        t = mixup_ref.target(labels, V, lam, smoothing)
        assert t.dtype == np.float32 and t.shape == want.shape and np.array_equal(t, want)


@pytest.mark.parametrize("tag", list(mixup_ref.CASES))
def test_mirror_mixup_on_cpu_draws_and_mixes_like_the_reference(z, tag):
    from focus_amd.slowfast.datasets import mixup as mx
    x, labels = case_inputs(z, tag)
    m = mx.MixUp(**mixup_ref.case_args(tag))
    seed = int(z[tag + ".seed"])
    np.random.seed(seed)                                                  # the draws alone, in the class's own order
    lam, use_cutmix = m._get_mixup_params()
    assert lam == float(z[tag + ".lam_drawn"]) and int(use_cutmix) == int(z[tag + ".cutmix"])
    if use_cutmix and lam != 1.0:
        box, lam = mx.get_cutmix_bbox(x.shape, lam, correct_lam=m.correct_lam)
        assert tuple(int(v) for v in box) == tuple(int(v) for v in z[tag + ".box"])
    assert float(lam) == float(z[tag + ".lam"])
    np.random.seed(seed)                                                  # the whole call
    got, tgt = m(x, labels)
    assert got is x and np.array_equal(x.numpy(), z[tag + ".clip"])
    if tag == "ek_dict":
        assert set(tgt) == {"verb", "noun"}
        for k in tgt:
            assert tgt[k].dtype == torch.float32 and np.array_equal(tgt[k].numpy(), z[tag + ".target." + k])
    else:
        assert tgt.dtype == torch.float32 and np.array_equal(tgt.numpy(), z[tag + ".target"])


def test_mirror_mixup_keeps_the_batch_size_assert():
    from focus_amd.slowfast.datasets.mixup import MixUp
    with pytest.raises(AssertionError, match="greater than 1"):
        MixUp(num_classes=5)(torch.zeros(1, 3, 2, 4, 4), torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("lam", [0.5, 1e-4, 1.0 - 1e-4, 0.3719, 0.5315061016529674])
@pytest.mark.parametrize("B", [2, 3])
def test_bf16_twin_equals_atens_three_bf16_operations(lam, B):
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, 3, 2, 5, 7, generator=g) * 3).to(torch.bfloat16)
    want = x.clone()
    flipped = want.flip(0).mul_(1.0 - lam)
    want.mul_(lam).add_(flipped)
    assert torch.equal(mixup_ref.blend(x, lam), want)
    x32 = x.float() * 1.0009765625                                        # fp32 values that are not bf16 values
    want = x32.clone()
    flipped = want.flip(0).mul_(1.0 - lam)
    want.mul_(lam).add_(flipped)
    assert torch.equal(mixup_ref.blend(x32, lam), want)


def test_soft_ce_twin_is_the_reference_expression():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 11, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.rand(3, 11, generator=g, dtype=torch.float64)
    loss = torch.sum(-y * torch.nn.functional.log_softmax(x, dim=-1), dim=-1)     # losses.py:30
    loss.mean().backward()
    ref_loss, ref_grad = mixup_ref.soft_ce(x, y)
    assert torch.allclose(ref_loss, loss.detach(), rtol=1e-13, atol=0) and torch.allclose(ref_grad, x.grad, rtol=1e-12, atol=1e-15)


def test_mixup_entry_points_validate_before_launching(built):
    """NULL pointers, bad sizes, bad rectangles and bad dtypes come back as the ABI's error codes before any launch."""
    from focus_amd import _lib
    lib = _lib.lib()
    F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr = ctypes.c_void_p(a)
    assert lib.focus_mixup_blend(None, 2, 64, 0.5, 0.5, F32, None) == NULL
    assert lib.focus_mixup_blend(ptr, 0, 64, 0.5, 0.5, F32, None) == SHAPE
    assert lib.focus_mixup_blend(ptr, -3, 64, 0.5, 0.5, BF16, None) == SHAPE
    assert lib.focus_mixup_blend(ptr, 2, 0, 0.5, 0.5, F32, None) == SHAPE
    assert lib.focus_mixup_blend(ptr, 2, 64, 0.5, 0.5, FP8, None) == DTYPE
    assert lib.focus_mixup_blend(ptr, 2, 64, 0.5, 0.5, 7, None) == DTYPE
    assert lib.focus_cutmix_paste(None, 2, 3, 8, 8, 1, 2, 1, 2, F32, None) == NULL
    assert lib.focus_cutmix_paste(ptr, 0, 3, 8, 8, 1, 2, 1, 2, F32, None) == SHAPE
    assert lib.focus_cutmix_paste(ptr, 2, 0, 8, 8, 1, 2, 1, 2, F32, None) == SHAPE
    assert lib.focus_cutmix_paste(ptr, 2, 3, 0, 8, 0, 0, 1, 2, F32, None) == SHAPE
    for yl, yh, xl, xh in [(-1, 2, 1, 2), (1, 9, 1, 2), (3, 2, 1, 2), (1, 2, -1, 2), (1, 2, 1, 9), (1, 2, 3, 2)]:
        assert lib.focus_cutmix_paste(ptr, 2, 3, 8, 8, yl, yh, xl, xh, BF16, None) == SHAPE
    assert lib.focus_cutmix_paste(ptr, 2, 3, 8, 8, 1, 2, 1, 2, FP8, None) == DTYPE
    assert lib.focus_cutmix_paste(ptr, 2, 3, 8, 8, 2, 2, 1, 5, F32, None) == 0          # empty rectangle: nothing to launch
    assert lib.focus_cutmix_paste(ptr, 2, 3, 8, 8, 1, 5, 8, 8, BF16, None) == 0
    assert lib.focus_mixup_target(None, ptr, 2, 5, 0.9, 0.02, 0.5, 0.5, None) == NULL
    assert lib.focus_mixup_target(ptr, None, 2, 5, 0.9, 0.02, 0.5, 0.5, None) == NULL
    assert lib.focus_mixup_target(ptr, ptr, 0, 5, 0.9, 0.02, 0.5, 0.5, None) == SHAPE
    assert lib.focus_mixup_target(ptr, ptr, 2, 0, 0.9, 0.02, 0.5, 0.5, None) == SHAPE
    for k in range(4):
        args = [ptr, ptr, ptr, ptr]
        args[k] = None
        assert lib.focus_xent_soft(*args, 2, 5, None) == NULL
    assert lib.focus_xent_soft(ptr, ptr, ptr, ptr, 0, 5, None) == SHAPE
    assert lib.focus_xent_soft(ptr, ptr, ptr, ptr, 2, 0, None) == SHAPE


def test_mixup_operators_refuse_cpu_tensors(built):
    from focus_amd import ops
    x = torch.randn(2, 3, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mixup_blend_(x, 0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cutmix_paste_(x, 0, 2, 0, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mixup_target(torch.tensor([0, 1]), 5, 0.3, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.soft_target_ce(torch.randn(2, 5), torch.rand(2, 5))


def test_library_exports_the_mixup_symbols(built):
    from focus_amd import _lib
    decl = _lib.parse_header()
    L = ctypes.CDLL(built)
    for name in ("focus_mixup_blend", "focus_cutmix_paste", "focus_mixup_target", "focus_xent_soft"):
        assert name in decl and hasattr(L, name), "missing: " + name
    for name in decl:
        assert hasattr(L, name), "missing export: " + name
    assert decl["focus_mixup_blend"][1] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_float,
                                            ctypes.c_int, ctypes.c_void_p]
    assert _lib.lib().focus_abi_version() == 2


def test_loss_lookup_returns_the_soft_losses():
    from focus_amd.slowfast.models import losses
    from focus_amd.slowfast.utils import misc
    cfg = get_cfg()
    assert cfg.MIXUP.ENABLE is False
    cfg.MODEL.LOSS_FUNC = "soft_cross_entropy"
    cfg.TRAIN.DATASET = "ssv2"
    loss = losses.get_loss_func(cfg)(reduction="mean")
    assert isinstance(loss, losses.SoftTargetCrossEntropy) and loss.reduction == "mean"
    assert isinstance(losses.get_loss_func(cfg, state="val")(reduction="mean"), losses.LabelSmoothingCrossEntropy)
    assert misc.get_num_classes(cfg) == cfg.MODEL.NUM_CLASSES
    cfg.TRAIN.DATASET = "epickitchens"
    ek = losses.get_loss_func(cfg)(reduction="mean")
    assert isinstance(ek, losses.EKLoss) and isinstance(ek.ce_loss, losses.SoftTargetCrossEntropy)
    assert isinstance(losses.get_loss_func(cfg, state="val")(reduction="mean").ce_loss, losses.LabelSmoothingCrossEntropy)
    assert misc.get_num_classes(cfg) == {"verb": 97, "noun": 300}


def test_build_mixup_follows_the_config():
    from focus_amd import train
    from focus_amd.slowfast.datasets.mixup import MixUp
    cfg = get_cfg()
    assert train.build_mixup(cfg) is None
    cfg.MIXUP.ENABLE = True
    m = train.build_mixup(cfg)
    assert isinstance(m, MixUp) and m.num_classes == cfg.MODEL.NUM_CLASSES
    assert (m.mixup_alpha, m.cutmix_alpha, m.mix_prob, m.switch_prob, m.label_smoothing) == (
        cfg.MIXUP.ALPHA, cfg.MIXUP.CUTMIX_ALPHA, cfg.MIXUP.PROB, cfg.MIXUP.SWITCH_PROB, cfg.MIXUP.LABEL_SMOOTH_VALUE)


def test_mixup_collapse_on_cpu_tensors():
    """Even B, labels[i] != labels[B-1-i], lam != 0.5, smoothing > 0: no ties in topk(labels, 2)."""
    from focus_amd import train
    g = torch.Generator().manual_seed(3)
    labels = np.array([3, 1, 4, 0], dtype=np.int64)
    dense = torch.from_numpy(mixup_ref.target(labels, 5, 0.37, 0.1))
    preds = torch.randn(4, 5, generator=g, requires_grad=True)
    got_p, got_l = train.mixup_collapse(preds, dense)
    want_p, want_l = mixup_ref.collapse(preds, dense)
    assert torch.equal(got_p, want_p) and torch.equal(got_l, want_l) and not got_p.requires_grad
    assert got_l.tolist() == [0, 4, 1, 3]                                 # lam < 0.5: the partner's class wins
    ek_l = {"verb": dense, "noun": torch.from_numpy(mixup_ref.target(np.array([299, 7, 8, 120]), 300, 0.8, 0.1))}
    ek_p = {"verb": preds, "noun": torch.randn(4, 300, generator=g)}
    got_p, got_l = train.mixup_collapse(ek_p, ek_l)
    for k in ek_l:
        want_p, want_l = mixup_ref.collapse(ek_p[k], ek_l[k])
        assert torch.equal(got_p[k], want_p) and torch.equal(got_l[k], want_l)
    assert got_l["noun"].tolist() == [299, 7, 8, 120]
