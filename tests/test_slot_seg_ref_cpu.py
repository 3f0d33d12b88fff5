"""No GPU: the twin of csrc/slot_segments.hip (tests/slot_seg_ref.py) and the mirror's box_ops.masks_to_boxes against the
fixture recorded from the reference (tests/golden/slot_boxes.npz, tests/make_slot_boxes_golden.py) and against the FG-ARI
fixture (tests/golden/metrics.npz); the mutants of the twin; the three symbols in the header and the library; and the
refusals the entry points judge before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import slot_seg_ref as ref
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(ref.GOLDEN, allow_pickle=False)


def case(gold, tag):
    B, T, He, We, K, sy, sx, _ = ref.CASES[tag]
    return gold[tag + ".attn"], gold[tag + ".seg"], gold[tag + ".boxes"], (B, T, He, We, K, sy, sx)


def orvit_of_recorded(boxes, H, W):
    """The project's own host chain on the recorded pixel boxes [B,T,K,4]."""
    from focus_amd.slowfast.datasets.utils import boxes_to_orvit_format
    return boxes_to_orvit_format(boxes, H, W).numpy()


@pytest.mark.parametrize("tag", list(ref.CASES))
def test_twin_and_mirror_match_the_reference(gold, tag):
    from focus_amd.slowfast.utils import box_ops
    attn, seg, boxes, (B, T, He, We, K, sy, sx) = case(gold, tag)
    assert attn.dtype == np.float32 and attn.shape == (B, T, He * We, K) and attn.nbytes < 100 * 1024
    assert (np.stack([(seg == k).sum(-1) for k in range(K)]) > 0).all()            # every slot owns a cell in every frame
    tseg, stats = ref.segments(attn, He, We)
    assert tseg.dtype == np.uint8 and np.array_equal(tseg, seg)
    px = ref.pixel_boxes(stats, sy, sx)
    assert px.dtype == boxes.dtype == np.float32 and np.array_equal(px, boxes)
    masks = torch.from_numpy(ref.upsampled_onehot(seg, He, We, K, sy, sx))
    mine = box_ops.masks_to_boxes(masks.flatten(end_dim=2)).reshape(B, T, K, 4)
    assert mine.dtype == torch.float32 and np.array_equal(mine.numpy(), boxes)
    H, W = He * sy, We * sx
    want = orvit_of_recorded(boxes, H, W)
    got = ref.to_orvit(px, H, W)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the whole of focus_slot_boxes with every slot kept: rows are the chain's rows, in slot order
    full, ids = ref.boxes(stats, He, We, H, W, K, drop_largest=False)
    assert np.array_equal(ids, np.tile(np.arange(K, dtype=np.int32), (B, 1)))
    assert np.array_equal(full.view(np.uint32), want.view(np.uint32))


def test_mirror_masks_to_boxes_edges():
    from focus_amd.slowfast.utils import box_ops
    assert tuple(box_ops.masks_to_boxes(torch.zeros(0, 4, 4)).shape) == (0, 4)
    m = torch.zeros(2, 5, 7)
    m[0, 1:3, 2:6] = 1
    m[1, 4, 0] = 1
    assert box_ops.masks_to_boxes(m).tolist() == [[2.0, 1.0, 5.0, 2.0], [0.0, 4.0, 0.0, 4.0]]


def test_the_thin_case_sits_on_the_edge_of_the_rule(gold):
    """Case "thin": slot 1's box is exactly fp32 0.05 wide, so `<=` makes it "no object" and its neighbour is kept."""
    attn, seg, boxes, (B, T, He, We, K, sy, sx) = case(gold, "thin")
    want = orvit_of_recorded(boxes, He * sy, We * sx)
    w1 = np.float32(boxes[0, 0, 1, 2]) / np.float32(We * sx) - np.float32(boxes[0, 0, 1, 0]) / np.float32(We * sx)
    assert w1 == np.float32(0.05)
    assert not want[0, 0, 1].any() and want[0, 0, 2].all() and want[0, 0, 0].all()


def test_selection_rule_by_hand():
    """Areas (5, 9, 9, 0, 3): the background is slot 1 (the lower of the two largest); of 0, 2, 4 the two largest are 2 and 0,
    written as 0, 2; slot 3 never counts."""
    stats = np.zeros((1, 2, 5, 5), dtype=np.int32)
    stats[0, 0, :, 0] = (5, 4, 9, 0, 1)
    stats[0, 1, :, 0] = (0, 5, 0, 0, 2)
    assert ref.select(stats, 2) == [[0, 2]]
    assert ref.select(stats, 2, mutant="area_order") == [[2, 0]]
    assert ref.select(stats, 2, mutant="keep_background") == [[1, 2]]
    assert ref.select(stats, 2, drop_largest=False) == [[1, 2]]
    assert ref.select(stats, 9) == [[0, 2, 4]] and ref.select(stats, 0) == [[]]
    stats[..., 1:] = (0, 0, 1, 1)
    b, ids = ref.boxes(stats, 4, 4, 16, 16, 4)
    assert ids.tolist() == [[0, 2, 4, -1]] and not b[0, :, 3].any()
    assert not b[0, 1, 0].any() and b[0, 0, 0].tolist() == [0.21875, 0.21875, 0.4375, 0.4375]    # slot 0 is absent in frame 1 only


def _expected(gold, tag, O):
    attn, seg, boxes, (B, T, He, We, K, sy, sx) = case(gold, tag)
    H, W = He * sy, We * sx
    rows = orvit_of_recorded(boxes, H, W)
    _, stats = ref.segments(attn, He, We)
    out = np.zeros((B, T, O, 4), dtype=np.float32)
    for b, kept in enumerate(ref.select(stats, O)):
        for o, k in enumerate(kept):
            out[b, :, o] = rows[b, :, k]
    return out, (attn, He, We, H, W)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_the_fixture_tells_the_mutants_apart(gold, mutant):
    """Each wrong rule, put into the twin, disagrees with what the recorded reference values give on some case; the twin
    itself agrees on all of them."""
    differs = False
    for tag in ref.CASES:
        O = 2
        want, (attn, He, We, H, W) = _expected(gold, tag, O)
        _, stats = ref.segments(attn, He, We)
        good, _ = ref.boxes(stats, He, We, H, W, O)
        assert np.array_equal(good.view(np.uint32), want.view(np.uint32)), tag
        mseg, mstats = ref.segments(attn, He, We, mutant)
        bad, _ = ref.boxes(mstats, He, We, H, W, O, mutant=mutant)
        differs |= not np.array_equal(bad, want) or not np.array_equal(mseg, gold[tag + ".seg"])
    assert differs, mutant


def test_twin_contingency_reproduces_the_reference_ari():
    """metrics.npz at scale 1: 1024 points = one 32x32 frame, 6 truth segments (row 0 = background), 7 slots."""
    z = np.load(os.path.join(GOLDEN, "metrics.npz"), allow_pickle=False)
    true, pred = z["true"], z["pred"]
    B, S, D = true.shape
    K = pred.shape[1]
    seg = np.argmax(pred, axis=1).astype(np.uint8).reshape(B, 1, D)
    truth = true.reshape(B, 1, S, 1, 32, 32)
    fg = ref.ari(ref.contingency(seg, truth, 32, 32, K, 1))
    assert np.abs(fg.numpy() - z["ari_each"]).max() < 1e-12
    assert abs(float(fg.sum() / B) - float(z["ari_fg"])) < 1e-12
    assert abs(float(ref.ari(ref.contingency(seg, truth, 32, 32, K, 0)).sum() / B) - float(z["ari_all"])) < 1e-12
    # and the table is the one evaluate_ari's matmul builds
    onehot = np.zeros_like(pred, dtype=np.int64)
    np.put_along_axis(onehot, np.argmax(pred, axis=1)[:, None], 1, axis=1)
    assert np.array_equal(ref.contingency(seg, truth, 32, 32, K, 0), (true != 0).astype(np.int64) @ onehot.transpose(0, 2, 1))


def test_twin_contingency_scales_and_overlap():
    g = np.random.RandomState(3)
    seg = g.randint(0, 3, (2, 2, 3 * 5)).astype(np.uint8)
    truth = (g.rand(2, 2, 4, 1, 6, 20) < 0.4).astype(np.float32)                       # overlapping, sy = 2, sx = 4
    truth[:, :, 2] = 0
    t = ref.contingency(seg, truth, 3, 5, 3, 1)
    assert t.shape == (2, 3, 3) and not t[:, 1].any()
    assert np.array_equal(t.sum(-1), (truth[:, :, 1:] != 0).sum(axis=(1, 3, 4, 5)))
    up = seg.reshape(2, 2, 3, 5)[:, :, np.arange(6) // 2][:, :, :, np.arange(20) // 4]
    assert t[1, 0, 2] == int(((truth[1, :, 1, 0] != 0) & (up[1] == 2)).sum())


# ---- the C ABI, no GPU -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


NAMES = ("focus_slot_segments", "focus_slot_boxes", "focus_seg_contingency")


def test_header_declares_and_library_exports(built):
    from focus_amd import _lib
    decl = _lib.parse_header()
    L = ctypes.CDLL(built)
    for n in NAMES:
        assert n in decl and hasattr(L, n), n
    assert len(decl["focus_slot_segments"][1]) == 10 and len(decl["focus_slot_boxes"][1]) == 13
    assert len(decl["focus_seg_contingency"][1]) == 14
    assert _lib.lib().focus_abi_version() == 2


def test_entry_points_refuse_before_launching(built):
    """Host pointers and no GPU: every refusal below is judged before a launch, and nothing is written."""
    from focus_amd import _lib, ops
    lib = _lib.lib()
    F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    NULL, SHAPE, DTYPE = -5, -1, -2
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    a += -a % 16
    p = ctypes.c_void_p(a)
    seg = lib.focus_slot_segments
    for i in (0, 7, 8):
        args = [p, F32, 1, 1, 4, 4, 3, p, p, None]
        args[i] = None
        assert seg(*args) == NULL, i
    for K, He, We in ((0, 4, 4), (33, 4, 4), (3, 0, 4), (3, 4, 0)):
        assert seg(p, F32, 1, 1, He, We, K, p, p, None) == SHAPE, (K, He, We)
    assert seg(p, FP8, 1, 1, 4, 4, 3, p, p, None) == DTYPE and seg(p, 7, 1, 1, 4, 4, 3, p, p, None) == DTYPE
    assert seg(p, BF16, 0, 5, 4, 4, 3, p, p, None) == 0 and seg(p, F32, 5, 0, 4, 4, 3, p, p, None) == 0     # B T == 0
    box = lib.focus_slot_boxes
    for i in (0, 10, 11):
        args = [p, 1, 1, 3, 4, 4, 16, 16, 2, 1, p, p, None]
        args[i] = None
        assert box(*args) == NULL, i
    assert box(p, 1, 1, 3, 4, 4, 16, 18, 2, 1, p, p, None) == SHAPE                     # W % We
    assert box(p, 1, 1, 3, 4, 4, 15, 16, 2, 1, p, p, None) == SHAPE                     # H % He
    assert box(p, 1, 1, 33, 4, 4, 16, 16, 2, 1, p, p, None) == SHAPE and box(p, 1, 1, 0, 4, 4, 16, 16, 2, 1, p, p, None) == SHAPE
    assert box(p, 0, 1, 3, 4, 4, 16, 16, 2, 1, p, p, None) == 0 and box(p, 1, 1, 3, 4, 4, 16, 16, 0, 1, p, p, None) == 0
    con = lib.focus_seg_contingency
    for i in (0, 1, 12):
        args = [p, p, 0, 1, 1, 3, 16, 16, 4, 4, 3, 1, p, None]
        args[i] = None
        assert con(*args) == NULL, i
    assert con(p, p, 0, 1, 1, 3, 16, 16, 4, 4, 3, 3, p, None) == SHAPE                  # S - first_segment < 1
    assert con(p, p, 0, 1, 1, 3, 16, 16, 4, 4, 33, 1, p, None) == SHAPE                 # K > 32
    assert con(p, p, 0, 1, 1, 3, 16, 18, 4, 4, 3, 1, p, None) == SHAPE                  # W % We
    assert con(p, p, 1, 1, 1, 3, 18, 16, 4, 4, 3, 1, p, None) == SHAPE                  # H % He
    assert con(p, p, 0, 1, 2, 3, 32768, 32768, 4, 4, 3, 1, p, None) == SHAPE            # T H W = 2^31
    assert con(p, p, 0, 1, 1, 3, 65536, 32768, 4, 4, 3, 1, p, None) == SHAPE
    assert con(p, p, 0, 0, 1, 3, 16, 16, 4, 4, 3, 1, p, None) == 0                      # B == 0
    assert bytes(buf) == bytes(1 << 12)
    x = torch.rand(1, 1, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.slot_segments(x, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.slot_boxes(torch.zeros(1, 1, 3, 5, dtype=torch.int32), 4, 4, 16, 16, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_contingency(torch.zeros(1, 1, 16, dtype=torch.uint8), torch.zeros(1, 1, 3, 1, 16, 16), 4, 4, 3)


def test_model_surface_without_a_gpu():
    """STEVE has segment / object_boxes, and they refuse the CPU like forward does; encode's path is the factored one."""
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import MODEL_REGISTRY
    from focus_amd.slowfast.utils import metrics
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "STEVE"
    s = cfg.SLOTS
    s.NUM_ITERS, s.NUM_SLOTS, s.CNN_HID_SIZE, s.SIZE, s.DIM, s.MLP_HID_SIZE, s.IMG_SIZE, s.VOCAB_SIZE = 2, 3, 8, 16, 16, 32, 16, 32
    s.NUM_PREDICTOR_BLOCKS, s.NUM_PREDICTOR_HEADS = 1, 2
    s.DECODER.DIM, s.DECODER.NUM_BLOCKS, s.DECODER.NUM_HEADS = 16, 1, 2
    m = MODEL_REGISTRY.get("STEVE")(cfg)
    assert m.orvit_objects == cfg.ORVIT.O
    for fn in (m.segment, m.object_boxes):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.rand(1, 2, 3, 16, 16))
    assert callable(metrics.evaluate_ari_segments)
