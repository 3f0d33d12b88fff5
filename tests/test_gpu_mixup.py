"""csrc/mixup.hip by the C ABI and by the operators above it: the blend and the target bit for bit against the twin of
tests/mixup_ref.py and the reference's recorded outputs (tests/golden/mixup.npz), the rectangle swap byte for byte, the
soft-target cross entropy against fp64 within the bounds the project holds focus_xent_ls to (tests/test_gpu_gumbel.py), and
the path end to end: MixUp.__call__ on the device, one train_iter step, mixup_collapse.

Shapes are the smallest that reach each hazard: 210 elements per sample (sample bases off 16 bytes in both dtypes: the
scalar path), 12288 per sample (16-byte accesses, and four trips of the grid-stride loop at the launch's block count), odd
batches (the middle sample pairs with itself in the blend and is left alone by the swap), 9x11 frames (scalar swap) and 16x16
frames (16-byte chunks, whole and cut by the rectangle's edge)."""
import ctypes

import numpy as np
import pytest
import torch

import mixup_ref
from conftest import load_golden
from focus_amd import _lib, ops

pytestmark = pytest.mark.gpu

CANARY = -768.0               # exact in bf16 too
PAD = 16                      # elements on both sides of the buffer: a multiple of 16 bytes in both dtypes
DTYPES = [torch.float32, torch.bfloat16]
LAMS = [0.5, 1e-4, 1.0 - 1e-4, 0.37, 0.5315061016529674]
LOSS_TOL, GRAD_TOL = 2e-5, {torch.float32: 1e-5, torch.bfloat16: 8e-3}      # tests/test_gpu_gumbel.py, focus_xent_ls


@pytest.fixture(scope="module")
def z():
    return mixup_ref.fixture()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def framed(x, shift=0):
    """x (CPU) inside a canary frame on the device -> (whole buffer, view of x's shape).  shift: extra elements before the
    view (a base that is not 16-byte aligned)."""
    n = x.numel()
    buf = torch.full((PAD + shift + n + PAD,), CANARY, dtype=x.dtype, device="cuda")
    view = buf[PAD + shift:PAD + shift + n].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (shift * x.element_size() % 16 == 0)
    return buf, view


def expect_framed(want, shift=0):
    """The buffer framed() would hold if its view held `want` (CPU)."""
    buf = torch.full((PAD + shift + want.numel() + PAD,), CANARY, dtype=want.dtype)
    buf[PAD + shift:PAD + shift + want.numel()] = want.reshape(-1)
    return buf


def clip(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 2.5).to(dtype)


# ---- blend ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,shift", [((2, 3, 2, 5, 7), 0), ((3, 3, 2, 5, 7), 0), ((4, 3, 2, 5, 7), 0),
                                         ((3, 3, 4, 32, 32), 0), ((4, 3, 4, 32, 32), 0), ((2, 3, 4, 32, 32), 1)])
def test_blend_equals_the_twin_bit_for_bit(shape, shift, dtype):
    x = clip(shape, dtype, seed=shape[0])
    B, n = shape[0], x[0].numel()
    for lam in LAMS:
        buf, view = framed(x, shift)
        status = _lib.lib().focus_mixup_blend(ctypes.c_void_p(view.data_ptr()), B, n, lam, 1.0 - lam,
                                              _lib.BF16 if dtype == torch.bfloat16 else _lib.F32, stream())
        torch.cuda.synchronize()
        assert status == 0
        want = mixup_ref.blend(x, lam)
        assert torch.equal(buf.cpu(), expect_framed(want, shift)), "lam %r" % lam
        if B % 2:                                                         # the middle sample is mixed with itself
            mid = x[B // 2].float()
            assert torch.equal(want[B // 2], mixup_ref.blend(torch.stack([mid, mid]).to(dtype), lam)[0])
            assert lam != 0.37 or not torch.equal(want[B // 2], x[B // 2])   # ... which is not the sample itself


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_blend_equals_atens_three_operations_on_the_device(dtype):
    """The reference's own sequence on the same device, the self-paired middle sample included."""
    x = clip((3, 3, 4, 32, 32), dtype, seed=7).cuda()
    for lam in LAMS:
        want = x.clone()
        flipped = want.flip(0).mul_(1.0 - lam)
        want.mul_(lam).add_(flipped)
        got = x.clone()
        assert ops.mixup_blend_(got, lam) is got
        assert torch.equal(got, want), "lam %r" % lam


def test_in_place_operators_refuse_what_they_cannot_mix_in_place():
    x = clip((2, 3, 2, 8, 8), torch.float32).cuda()
    with pytest.raises(ValueError, match="contiguous"):
        ops.mixup_blend_(x.transpose(1, 2), 0.3)
    with pytest.raises(ValueError, match="contiguous"):
        ops.cutmix_paste_(x[..., ::2], 0, 2, 0, 2)
    with pytest.raises(ValueError, match="outside"):
        ops.cutmix_paste_(x, 0, 9, 0, 2)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        ops.mixup_blend_(x.half(), 0.3)
    keep = x.clone()
    assert ops.cutmix_paste_(x, 3, 3, 0, 8) is x and torch.equal(x, keep)


# ---- cutmix -----------------------------------------------------------------------------------------------------------
def boxes_of(H, W):
    return {"one_pixel": (H // 2, H // 2 + 1, W // 2, W // 2 + 1), "odd_xl_odd_width": (2, 7, 3, 8),
            "right_bottom_edge": (H - 3, H, 5, W), "left_top_edge": (0, 2, 0, 3), "full_frame": (0, H, 0, W),
            "empty_rows": (3, 3, 2, 6), "empty_columns": (1, 5, W, W)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("tail", [(3, 2, 9, 11), (2, 3, 16, 16)], ids=["BCTHW_9x11", "BTCHW_16x16"])
def test_cutmix_swaps_the_rectangle_and_nothing_else(tail, B, dtype):
    x = clip((B,) + tail, dtype, seed=B)
    H, W = tail[-2:]
    for name, (yl, yh, xl, xh) in boxes_of(H, W).items():
        buf, view = framed(x)
        status = _lib.lib().focus_cutmix_paste(ctypes.c_void_p(view.data_ptr()), B, tail[0] * tail[1], H, W, yl, yh, xl, xh,
                                               _lib.BF16 if dtype == torch.bfloat16 else _lib.F32, stream())
        torch.cuda.synchronize()
        assert status == 0, name
        want = mixup_ref.paste(x, yl, yh, xl, xh)
        assert torch.equal(buf.cpu(), expect_framed(want)), name          # the rectangle, its surroundings and the canaries
        if name.startswith("empty"):
            assert torch.equal(want, x)
        if name == "full_frame" and B == 2:                               # the in-place hazard: an exact swap
            assert torch.equal(view[0].cpu(), x[1]) and torch.equal(view[1].cpu(), x[0])
        if B == 3:
            assert torch.equal(view[1].cpu(), x[1])                       # the middle sample stays
        got = x.cuda()
        assert ops.cutmix_paste_(got, yl, yh, xl, xh) is got and torch.equal(got.cpu(), want), name


def test_cutmix_on_an_unaligned_base_takes_the_scalar_path():
    x = clip((2, 2, 3, 16, 16), torch.float32, seed=5)
    buf, view = framed(x, shift=1)
    assert _lib.lib().focus_cutmix_paste(ctypes.c_void_p(view.data_ptr()), 2, 6, 16, 16, 2, 9, 3, 16, _lib.F32, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), expect_framed(mixup_ref.paste(x, 2, 9, 3, 16), shift=1))


# ---- target -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [5, 174, 300])
@pytest.mark.parametrize("labels", [[1, 4], [2, 2], [3, 0, 4], [4, 1, 4]], ids=["B2", "B2_equal", "B3", "B3_equal"])
def test_target_equals_the_twin_bit_for_bit(labels, V):
    lab = np.array(labels, dtype=np.int64)
    dev_lab = torch.from_numpy(lab).cuda()
    for smoothing in (0.0, 0.1):
        for lam in LAMS + [1.0]:
            got = ops.mixup_target(dev_lab, V, lam, smoothing)
            assert got.dtype == torch.float32 and got.shape == (len(labels), V)
            assert np.array_equal(got.cpu().numpy(), mixup_ref.target(lab, V, lam, smoothing)), (smoothing, lam)
    assert np.array_equal(ops.mixup_target(dev_lab.int(), V, 0.37, 0.1).cpu().numpy(), mixup_ref.target(lab, V, 0.37, 0.1))


def test_target_equals_the_reference_recorded_targets(z):
    for tag in mixup_ref.CASES:
        B = mixup_ref.CASES[tag][0]
        smoothing = mixup_ref.case_args(tag).get("label_smoothing", 0.1)
        heads = {".target." + k: ("ek." + k, mixup_ref.EK_CLASSES[k]) for k in ("verb", "noun")} if tag == "ek_dict" else \
            {".target": ("labels", mixup_ref.NUM_CLASSES)}
        for suffix, (lab, V) in heads.items():
            got = ops.mixup_target(torch.from_numpy(z[lab][:B].copy()).cuda(), V, float(z[tag + ".lam"]), smoothing)
            assert np.array_equal(got.cpu().numpy(), z[tag + suffix]), tag + suffix


def test_target_with_labels_outside_the_classes_stays_inside_its_buffer():
    """A label outside [0,V) matches no column: its row holds `off` wherever the partner's label is not, nothing is stored
    outside [B,V]."""
    V, lab = 5, np.array([-1, 5, 2], dtype=np.int64)
    buf, view = framed(torch.zeros(3, V))
    on, off = 1.0 - 0.1 + 0.1 / V, 0.1 / V
    status = _lib.lib().focus_mixup_target(ctypes.c_void_p(torch.from_numpy(lab).cuda().data_ptr()),
                                           ctypes.c_void_p(view.data_ptr()), 3, V, on, off, 0.37, 1.0 - 0.37, stream())
    torch.cuda.synchronize()
    assert status == 0
    want = torch.from_numpy(mixup_ref.target(lab, V, 0.37, 0.1))
    assert torch.equal(buf.cpu(), expect_framed(want))
    assert torch.equal(want[1], torch.full((V,), float(want[1, 0])))      # both labels of the middle row are outside


# ---- soft-target cross entropy --------------------------------------------------------------------------------------------
def ce_variants(R, V):
    """name -> (logits fp32 [R,V], target fp32 [R,V]) on the device; the targets start from mixup_target rows."""
    g = torch.Generator().manual_seed(100 * R + V)
    labels = torch.randint(0, V, (R,), generator=g).cuda()
    y = ops.mixup_target(labels, V, 0.37, 0.1)
    x = torch.randn(R, V, generator=g).cuda() * 3
    big = x / x.abs().max() * 80 if V > 1 else torch.full_like(x, 80.0)
    part = y.clone()
    part[0] *= 0.7
    part[0, V // 2] += 0.25                                               # a row that does not sum to 1
    zero = y.clone()
    zero[0] = 0.0                                                         # an all-zero row: loss 0, gradient 0
    return {"mixup_target": (x, y), "not_sum_1": (x, part), "zero_row": (x, zero), "logits_80": (big, y), "logits_80_part": (-big, part)}


def check_ce(x, y, got_loss, got_grad, dtype, what):
    ref_loss, ref_grad = mixup_ref.soft_ce(x, y)
    got_loss, got_grad = got_loss.detach().double().cpu(), got_grad.detach().double().cpu()
    err = (got_loss - ref_loss).abs()
    bound = LOSS_TOL * ref_loss.abs().clamp(min=1.0)
    print("%s: loss err/bound %.3g, grad err %.3g bound %.3g" % (what, float((err / bound).max()),
                                                                 float((got_grad - ref_grad).abs().max()),
                                                                 GRAD_TOL[dtype] * float(ref_grad.abs().max())))
    assert torch.isfinite(got_loss).all() and torch.isfinite(got_grad).all(), what
    assert bool((err <= bound).all()), (what, got_loss, ref_loss)
    assert float((got_grad - ref_grad).abs().max()) <= GRAD_TOL[dtype] * float(ref_grad.abs().max()), what
    return ref_loss, ref_grad


@pytest.mark.parametrize("V", [1, 5, 174, 257, 1000])
@pytest.mark.parametrize("R", [1, 3])
def test_soft_ce_kernel_against_fp64(R, V):
    """focus_xent_soft by the C ABI: loss rows and d(mean)/d(logits), canaries around both outputs."""
    for name, (x, y) in ce_variants(R, V).items():
        lbuf, loss = framed(torch.zeros(R))
        gbuf, grad = framed(torch.zeros(R, V))
        status = _lib.lib().focus_xent_soft(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                            ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(grad.data_ptr()), R, V, stream())
        torch.cuda.synchronize()
        assert status == 0
        what = "R%d V%d %s" % (R, V, name)
        check_ce(x, y, loss, grad, torch.float32, what)
        for b, n in ((lbuf, R), (gbuf, R * V)):
            c = b.cpu()
            assert bool((c[:PAD] == CANARY).all()) and bool((c[PAD + n:] == CANARY).all()), what
        if name == "zero_row":
            assert float(loss[0]) == 0.0 and not bool(grad[0].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,V", [(3, 5), (3, 257), (1, 1000)])
def test_soft_target_ce_operator_mean_and_none(R, V, dtype):
    for name, (x, y) in ce_variants(R, V).items():
        x = x.to(dtype)
        what = "R%d V%d %s %s" % (R, V, name, dtype)
        leaf = x.clone().requires_grad_()
        loss = ops.soft_target_ce(leaf, y)                                # reduction="mean"
        loss.backward()
        assert loss.dim() == 0 and loss.dtype == torch.float32 and leaf.grad.dtype == dtype
        ref_loss, ref_grad = mixup_ref.soft_ce(x, y)
        assert abs(float(loss.detach()) - float(ref_loss.mean())) <= LOSS_TOL * max(1.0, abs(float(ref_loss.mean()))), what
        assert float((leaf.grad.double().cpu() - ref_grad).abs().max()) <= GRAD_TOL[dtype] * float(ref_grad.abs().max()), what
        # reduction="none": the rows, and a non-uniform incoming gradient scales the rows of d(logits)
        leaf = x.clone().requires_grad_()
        rows = ops.soft_target_ce(leaf, y, reduction="none")
        w = torch.linspace(0.5, 2.0, R, device="cuda")
        (rows * w).sum().backward()
        want_grad = ref_grad * R * w.double().cpu()[:, None]
        assert rows.shape == (R,) and bool(((rows.double().cpu() - ref_loss).abs() <= LOSS_TOL * ref_loss.abs().clamp(min=1.0)).all()), what
        assert float((leaf.grad.double().cpu() - want_grad).abs().max()) <= GRAD_TOL[dtype] * float(want_grad.abs().max()), what


def test_soft_target_loss_modules_run_on_the_operator():
    from focus_amd.slowfast.models import losses
    x, y = ce_variants(3, 174)["mixup_target"]
    ref_loss, _ = mixup_ref.soft_ce(x, y)
    got = losses.SoftTargetCrossEntropy(reduction="mean")(x, y)
    assert abs(float(got) - float(ref_loss.mean())) <= LOSS_TOL * max(1.0, float(ref_loss.mean()))
    rows = losses.SoftTargetCrossEntropy(reduction="none")(x, y)
    assert rows.shape == (3,)
    ek = losses.EKLoss(reduction="mean", ce_type="soft")({"verb": x, "noun": x}, {"verb": y, "noun": y})
    assert float(ek["verb_loss"]) == float(got) and float(ek["noun_loss"]) == float(got)
    with pytest.raises(ValueError, match="reduction"):
        ops.soft_target_ce(x, y, reduction="sum")


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(mixup_ref.CASES))
def test_mixup_call_on_the_device_equals_the_reference(z, tag):
    """The reference's recorded cases through MixUp.__call__ on device tensors, seeded as recorded."""
    from focus_amd.slowfast.datasets.mixup import MixUp
    B = mixup_ref.CASES[tag][0]
    x = torch.from_numpy(z["x"][:B].copy()).cuda()
    if tag == "ek_dict":
        labels = {k: torch.from_numpy(z["ek." + k][:B].copy()).cuda() for k in ("verb", "noun")}
    else:
        labels = torch.from_numpy(z["labels"][:B].copy()).cuda()
    np.random.seed(int(z[tag + ".seed"]))
    got, tgt = MixUp(**mixup_ref.case_args(tag))(x, labels)
    assert got is x and np.array_equal(x.cpu().numpy(), z[tag + ".clip"])
    if tag == "ek_dict":
        assert set(tgt) == {"verb", "noun"}
        for k in tgt:
            assert tgt[k].is_cuda and np.array_equal(tgt[k].cpu().numpy(), z[tag + ".target." + k])
    else:
        assert tgt.is_cuda and np.array_equal(tgt.cpu().numpy(), z[tag + ".target"])


def test_mixup_collapse_on_the_device_equals_the_reference_lines():
    """Even B, labels[i] != labels[B-1-i], lam != 0.5 and smoothing > 0 leave no ties in topk(labels, 2)."""
    from focus_amd import train
    g = torch.Generator().manual_seed(3)
    labels = torch.tensor([3, 1, 4, 0]).cuda()
    dense = ops.mixup_target(labels, 5, 0.37, 0.1)
    preds = torch.randn(4, 5, generator=g).cuda().requires_grad_()
    got_p, got_l = train.mixup_collapse(preds, dense)
    want_p, want_l = mixup_ref.collapse(preds, dense)
    assert got_p.is_cuda and not got_p.requires_grad and torch.equal(got_p.cpu(), want_p) and torch.equal(got_l.cpu(), want_l)
    assert got_l.tolist() == [0, 4, 1, 3]
    ek_l = {"verb": dense, "noun": ops.mixup_target(torch.tensor([299, 7, 8, 120]).cuda(), 300, 0.8, 0.1)}
    ek_p = {"verb": preds, "noun": torch.randn(4, 300, generator=g).cuda()}
    got_p, got_l = train.mixup_collapse(ek_p, ek_l)
    for k in ek_l:
        want_p, want_l = mixup_ref.collapse(ek_p[k], ek_l[k])
        assert torch.equal(got_p[k].cpu(), want_p) and torch.equal(got_l[k].cpu(), want_l)


def test_train_iter_with_mixup_and_the_soft_loss():
    """One train_iter step of the small ORViT-Motionformer (the configuration of tests/test_gpu_parity.py) with MIXUP.ENABLE,
    soft_cross_entropy and B = 2: the clips are mixed in place as the twin says, the loss is the fp64 soft CE of the step's
    logits against the twin's target, every parameter gets a finite gradient, and the returned predictions and labels are
    the collapsed ones."""
    from focus_amd import train
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.datasets import mixup as mx
    from focus_amd.slowfast.models import build_model
    from focus_amd.slowfast.models.losses import SoftTargetCrossEntropy, get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    a, p = load_golden("motionformer_small")
    cfg = get_cfg()
    cfg.merge_from_list(["ORVIT.ENABLE", True, "ORVIT.O", 3, "ORVIT.LAYERS", [1], "DATA.TRAIN_CROP_SIZE", 64,
                         "DATA.NUM_FRAMES", 4, "MF.EMBED_DIM", 64, "MF.DEPTH", 3, "MF.NUM_HEADS", 4,
                         "MF.TEMPORAL_RESOLUTION", 2, "MF.USE_MLP", True, "MODEL.NUM_CLASSES", 10,
                         "MODEL.MODEL_NAME", "Motionformer", "TRAIN.DATASET", "Ssv2", "NUM_GPUS", 1,
                         "TRAIN.MIXED_PRECISION", False, "MODEL.LOSS_FUNC", "soft_cross_entropy", "MIXUP.ENABLE", True,
                         "SOLVER.OPTIMIZING_METHOD", "adamw", "SOLVER.BASE_LR", 1e-3, "SOLVER.CLIP_GRAD_L2NORM", 1.0])
    m = build_model(cfg)
    m.load_state_dict({k: v.float() for k, v in p.items()})
    m.train()
    opt = construct_optimizer(m, cfg)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    mixup_fn = train.build_mixup(cfg)
    assert isinstance(loss_fun, SoftTargetCrossEntropy) and isinstance(mixup_fn, mx.MixUp)
    x0 = torch.from_numpy(a["x"])
    labels = torch.from_numpy(a["labels"])
    assert x0.shape[0] == 2 and int(labels[0]) != int(labels[1])

    seed = 0
    np.random.seed(seed)                                                  # what this seed draws, by the class's own functions
    lam, use_cutmix = mixup_fn._get_mixup_params()
    assert lam not in (1.0, 0.5)
    if use_cutmix:
        box, lam = mx.get_cutmix_bbox(x0.shape, lam, correct_lam=mixup_fn.correct_lam)
        want_x = mixup_ref.paste(x0, *[int(v) for v in box])
    else:
        want_x = mixup_ref.blend(x0, lam)
    want_y = torch.from_numpy(mixup_ref.target(a["labels"], cfg.MODEL.NUM_CLASSES, lam, cfg.MIXUP.LABEL_SMOOTH_VALUE))
    assert float(lam) not in (1.0, 0.5)

    seen = []
    hook = m.register_forward_hook(lambda _m, _i, out: seen.append((out[0] if isinstance(out, tuple) else out).detach().clone()))
    x = x0.clone().cuda()
    inputs = [x]
    np.random.seed(seed)
    preds, out_labels, loss = train.train_iter(m, opt, loss_fun, inputs, labels.cuda(), {"orvit_bboxes": torch.from_numpy(a["boxes"]).cuda()},
                                               cfg, mixup_fn=mixup_fn)
    hook.remove()
    assert inputs[0] is x and torch.equal(x.cpu(), want_x)                # mixed in place, with the twin's bits
    assert len(seen) == 1 and seen[0].shape == (2, cfg.MODEL.NUM_CLASSES)
    ref_loss = float(mixup_ref.soft_ce(seen[0], want_y)[0].mean())
    print("train_iter loss %.7f, fp64 soft CE of its logits %.7f" % (float(loss), ref_loss))
    assert np.isfinite(float(loss)) and abs(float(loss) - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss))
    for name, prm in m.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
    want_p, want_l = mixup_ref.collapse(seen[0], want_y)
    assert torch.equal(preds.cpu(), want_p) and torch.equal(out_labels.cpu(), want_l) and not preds.requires_grad
    # without a mixup function the iteration is train_step plus the labels it was given
    cfg.MODEL.LOSS_FUNC = "cross_entropy"
    hard = labels.cuda()
    preds, out_labels, loss = train.train_iter(m, opt, get_loss_func(cfg)(reduction="mean"), [x0.clone().cuda()], hard,
                                               {"orvit_bboxes": torch.from_numpy(a["boxes"]).cuda()}, cfg)
    assert out_labels is hard and preds.shape == (2, cfg.MODEL.NUM_CLASSES) and np.isfinite(float(loss))


def test_train_iter_with_the_epic_kitchens_label_dict():
    """The dict branch: verb / noun labels mixed with their own class counts, EKLoss on the soft loss, and both heads'
    predictions collapsed (train_step itself hands back the verb logits only).  Two Linear heads stand in for the model."""
    from focus_amd import train
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models.losses import EKLoss, get_loss_func

    class TwoHeads(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.verb, self.noun = torch.nn.Linear(12, 97), torch.nn.Linear(12, 300)

        def forward(self, inputs, meta=None):
            f = inputs[0].flatten(1)[:, :12]
            v, n = self.verb(f), self.noun(f)
            return v, {"verb": v, "noun": n}

    cfg = get_cfg()
    cfg.merge_from_list(["TRAIN.DATASET", "epickitchens", "MODEL.LOSS_FUNC", "soft_cross_entropy", "MIXUP.ENABLE", True])
    torch.manual_seed(0)
    m = TwoHeads().cuda()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    mixup_fn = train.build_mixup(cfg)
    assert isinstance(loss_fun, EKLoss) and mixup_fn.num_classes == {"verb": 97, "noun": 300}
    x0 = clip((4, 3, 2, 8, 8), torch.float32, seed=9)
    lab = {"verb": np.array([5, 96, 0, 41], dtype=np.int64), "noun": np.array([299, 7, 8, 120], dtype=np.int64)}
    np.random.seed(0)
    lam, use_cutmix = mixup_fn._get_mixup_params()
    assert not use_cutmix and lam not in (1.0, 0.5)
    want_y = {k: torch.from_numpy(mixup_ref.target(v, mixup_fn.num_classes[k], lam, cfg.MIXUP.LABEL_SMOOTH_VALUE)) for k, v in lab.items()}
    seen = {}
    hook = m.register_forward_hook(lambda _m, _i, out: seen.update({k: v.detach().clone() for k, v in out[1].items()}))
    x = x0.clone().cuda()
    np.random.seed(0)
    preds, labels, loss = train.train_iter(m, opt, loss_fun, [x], {k: torch.from_numpy(v).cuda() for k, v in lab.items()}, {}, cfg,
                                           mixup_fn=mixup_fn)
    hook.remove()
    assert torch.equal(x.cpu(), mixup_ref.blend(x0, lam))
    ref = sum(float(mixup_ref.soft_ce(seen[k], want_y[k])[0].mean()) for k in lab)
    assert np.isfinite(float(loss)) and abs(float(loss) - ref) <= 2 * LOSS_TOL * max(1.0, ref)      # the sum of two bounded losses
    assert set(preds) == set(labels) == {"verb", "noun"}
    for k in lab:
        want_p, want_l = mixup_ref.collapse(seen[k], want_y[k])
        assert torch.equal(preds[k].cpu(), want_p) and torch.equal(labels[k].cpu(), want_l)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
