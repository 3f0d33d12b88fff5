"""No GPU: the twin of csrc/multilabel.hip (tests/multilabel_ref.py) and the host side of the multi-label route against the
fixture recorded from the reference (tests/golden/multilabel.npz: get_map, TestMeter(multi_label=True), torch's two BCE
losses) and, where it can be imported, against scikit-learn itself; the twin's two forms of average precision against each
other; its mutants; the new symbols' refusals through the built library; the losses' lookup, the config keys, the label
helpers, and meters.MultiLabelStats on two gloo ranks."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import multilabel_ref as ref

AP_CASES = ("ties", "zero_class", "one_class", "single_kept", "fill", "nan", "none_kept", "random300", "all_equal")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "multilabel.npz")))


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


# ---- average precision -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AP_CASES)
def test_twin_and_host_get_map_equal_the_recorded_reference(gold, case):
    from focus_amd.slowfast.utils import meters
    s, y, want = gold["ap.%s.scores" % case], gold["ap.%s.labels" % case], float(gold["ap.%s.map" % case])
    N, C = s.shape
    ap, npos, summary, flag = ref.average_precision_counting(s, y)
    twin, host = ref.get_map_twin(s, y), float(meters.get_map(s, y))
    print(case, "twin - ref %.3g" % (twin - want), "host - ref %.3g" % (host - want), "bound %.3g" % ref.map_bound(N, C))
    assert abs(twin - want) <= ref.map_bound(N, C) and abs(host - want) <= ref.map_bound(N, C)
    assert float(meters.get_map(torch.from_numpy(s), torch.from_numpy(y))) == host           # CPU tensors: the same path
    assert np.array_equal(npos, (y != 0).sum(0))
    kept = npos > 0
    assert summary[1] == kept.sum() and not ap[~kept].any()
    assert flag == {"nan": ref.BAD_SCORE, "none_kept": ref.NO_CLASS}.get(case, 0)
    if "ap.%s.aps" % case in gold:
        aps = gold["ap.%s.aps" % case]
        assert np.abs(ap[kept] - aps).max() <= ref.ap_bound(N)
        sort = np.array([ref.average_precision_sorting(s[:, c], y[:, c]) for c in np.nonzero(kept)[0]])
        print(case, "counting - sklearn %.3g" % np.abs(ap[kept] - aps).max(), "counting - sorting %.3g" % np.abs(ap[kept] - sort).max())
        assert np.abs(ap[kept] - sort).max() <= ref.ap_bound(N)


def test_twin_and_host_get_map_against_scikit_learn_directly():
    sk = pytest.importorskip("sklearn.metrics")
    from focus_amd.slowfast.utils import meters
    g = np.random.RandomState(0)
    worst = 0.0
    for _ in range(40):
        N, C = int(g.randint(1, 330)), int(g.randint(1, 9))
        s = np.round(g.randn(N, C), int(g.randint(0, 3))).astype(np.float32)                  # heavy ties
        y = (g.rand(N, C) < g.choice([0.05, 0.3, 0.9])).astype(np.float32)
        s[g.rand(N) < 0.2] = -1e10
        kept = ~np.all(y == 0, axis=0)
        if not kept.any():
            assert meters.get_map(s, y) == 0.0 and ref.get_map_twin(s, y) == 0.0
            continue
        want = sk.average_precision_score(y[:, kept], s[:, kept], average=None)
        ap, npos, summary, flag = ref.average_precision_counting(s, y)
        assert flag == 0 and np.array_equal(npos > 0, kept)
        d = np.abs(ap[kept] - want).max()
        worst = max(worst, d / ref.ap_bound(N))
        assert d <= ref.ap_bound(N)
        assert abs(float(meters.get_map(s, y)) - np.mean(want)) <= ref.map_bound(N, C)
        assert abs(summary[0] - np.mean(want)) <= ref.map_bound(N, C)
    print("worst counting - sklearn, as a share of the bound: %.3g" % worst)


def test_get_map_refuses_labels_that_are_not_binary():
    from focus_amd.slowfast.utils import meters
    s, y = np.float32([[0.1, 0.2], [0.3, 0.4]]), np.float32([[1, 0], [0.5, 0]])
    with pytest.raises(ValueError, match="0 or 1"):
        meters.get_map(s, y)
    assert ref.average_precision_counting(s, y)[3] == ref.BAD_LABEL
    assert meters.get_map(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)) == 0.0
    assert ref.average_precision_counting(np.float32([[np.inf]]), np.float32([[1]]))[3] == ref.BAD_SCORE


def test_hand_worked_average_precision():
    # scores 3 2 2 1, labels 1 0 1 1: thresholds 3 (1/1), 2 (2/3), 1 (3/4); positives at them 1, 1, 1 -> (1 + 2/3 + 3/4) / 3
    s, y = np.float32([[2], [3], [1], [2]]), np.float32([[1], [1], [1], [0]])
    cnt, tp = ref.ap_counts(s[:, 0], y[:, 0])
    assert cnt.tolist() == [3, 1, 4, 3] and tp.tolist() == [2, 1, 3, 2]
    want = (1 + 2 / 3 + 3 / 4) / 3
    assert abs(ref.average_precision_counting(s, y)[0][0] - want) < 1e-15
    assert abs(ref.average_precision_sorting(s[:, 0], y[:, 0]) - want) < 1e-15


@pytest.mark.parametrize("mutant,cases", [("gt_count", ("ties", "fill", "all_equal")), ("index_ties", ("ties", "fill", "all_equal")),
                                          ("divide_by_n", ("ties", "random300")), ("keep_zero_classes", ("zero_class", "single_kept"))])
def test_ap_mutants_leave_the_bound(gold, mutant, cases):
    for case in cases:
        s, y, want = gold["ap.%s.scores" % case], gold["ap.%s.labels" % case], float(gold["ap.%s.map" % case])
        b = ref.map_bound(*s.shape)
        d = abs(ref.get_map_twin(s, y, mutant) - want)
        print(mutant, case, "error / bound = %.3g" % (d / b))
        assert d > 100 * b


# ---- the meter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "sum"])
def test_host_test_meter_multi_label_equals_the_reference_bit_for_bit(gold, mode):
    from focus_amd.slowfast.utils import meters
    t = {k: gold["tm.%s.%s" % (mode, k)] for k in ("preds", "labels", "clip_ids", "splits", "video_preds", "video_labels",
                                                    "clip_count", "map")}
    nv, C = t["video_preds"].shape
    m = meters.TestMeter(nv, 3, C, len(t["splits"]), multi_label=True, ensemble_method=mode)
    assert (m.video_preds == -1e10).all() and m.video_labels.shape == (nv, C)
    vp, vl = np.full((nv, C), -1e10, np.float32), np.zeros((nv, C), np.float32)
    cc, flag, o = np.zeros(nv, np.int64), np.zeros(1, np.int32), 0
    for n in t["splits"]:
        sl = slice(o, o + n)
        m.update_stats(torch.from_numpy(t["preds"][sl]), torch.from_numpy(t["labels"][sl]), torch.from_numpy(t["clip_ids"][sl]))
        ref.view_accumulate_dense(t["preds"][sl], t["clip_ids"][sl], t["labels"][sl], 3, vp, vl, cc, flag, mode)
        o += n
    stats = m.finalize_metrics()
    for got_p, got_l, got_c in ((m.video_preds.numpy(), m.video_labels.numpy(), m.clip_count.numpy()), (vp, vl, cc)):
        assert np.array_equal(got_p.view(np.uint32), t["video_preds"].view(np.uint32))
        assert np.array_equal(got_l, t["video_labels"]) and np.array_equal(got_c, t["clip_count"])
    assert flag[0] == 0 and stats["complete"] and stats["split"] == "test_final"
    assert float(stats["map"]) == float(t["map"])
    if mode == "sum":
        assert (t["video_preds"] == -1e10).all()                # fp32 swallows every score added to -1e10
    m.reset()
    assert (m.video_preds == -1e10).all() and not m.video_labels.any() and not m.clip_count.any()
    with pytest.raises(AssertionError):
        bad = torch.from_numpy(t["labels"][:1].copy())
        bad[0] = 1 - bad[0]
        m.update_stats(torch.from_numpy(t["preds"][:1]), torch.from_numpy(t["labels"][:1]), torch.from_numpy(t["clip_ids"][:1]))
        m.update_stats(torch.from_numpy(t["preds"][:1]), bad, torch.from_numpy(t["clip_ids"][:1]))


def test_twin_view_fold_flags():
    vp, vl = np.full((2, 3), -1e10, np.float32), np.zeros((2, 3), np.float32)
    cc, flag = np.zeros(2, np.int64), np.zeros(1, np.int32)
    p = np.float32([[1, 2, 3], [3, 2, 1], [9, 9, 9]])
    ref.view_accumulate_dense(p, [0, 1, 4], np.float32([[1, 0, 0], [1, 0, 0], [1, 1, 1]]), 2, vp, vl, cc, flag, "max")
    assert flag[0] == 2 and cc.tolist() == [2, 0] and vp[0].tolist() == [3, 2, 3] and (vp[1] == -1e10).all()
    ref.view_accumulate_dense(p[:1], [1], np.float32([[0, 1, 0]]), 2, vp, vl, cc, flag, "max")
    assert flag[0] == 3 and vl[0].tolist() == [0, 1, 0]                                   # written either way


# ---- BCE -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,xk,yk", [("logits", "bce.x", "bce.y"), ("probs", "bce.p", "bce.yp")])
def test_bce_twin_against_torch_and_fp32_twin_inside_the_bound(gold, mode, xk, yk):
    x, y = gold[xk], gold[yk]
    name = "logit" if mode == "logits" else "prob"
    R, C = x.shape
    for red, gs in (("mean", 1.0 / (R * C)), ("sum", 1.0)):
        rows, dx, row_b, dx_b = ref.bce_rows(x, y, mode, gs)
        want, want_g = float(gold["bce.%s.f64.%s" % (name, red)]), gold["bce.%s.f64.grad_%s" % (name, red)]
        assert abs(rows.sum() * gs - want) <= 1e-13 * abs(want)
        assert np.allclose(dx, want_g, rtol=1e-7, atol=0)                   # 1e-12 as fp32 against 1e-12 as fp64 in the clamp
        w32, g32 = float(gold["bce.%s.f32.%s" % (name, red)]), gold["bce.%s.f32.grad_%s" % (name, red)].astype(np.float64)
        print(mode, red, "torch fp32 loss error / bound %.3g" % (abs(w32 - rows.sum() * gs) / (row_b.sum() * gs)),
              "grad %.3g" % (np.abs(g32 - dx) / dx_b).max())
        assert abs(w32 - rows.sum() * gs) <= row_b.sum() * gs and (np.abs(g32 - dx) <= dx_b).all()   # ATen's fp32 evaluation
    f32 = ref.bce_rows_fp32(x, y, mode).astype(np.float64)
    rows, _, row_b, _ = ref.bce_rows(x, y, mode)
    print(mode, "fp32 twin row error / bound", np.abs(f32 - rows) / row_b)
    assert (np.abs(f32 - rows) <= row_b).all() and np.isfinite(rows).all()


def test_bce_fp32_twin_inside_the_bound_on_wide_rows():
    g = np.random.RandomState(5)
    for C in (1, 157, 257, 1000):
        x, y = (g.randn(3, C) * 6).astype(np.float32), g.rand(3, C).astype(np.float32)
        rows, _, b, _ = ref.bce_rows(x, y, "logits")
        assert (np.abs(ref.bce_rows_fp32(x, y, "logits") - rows) <= b).all()
        p = g.rand(3, C).astype(np.float32)
        rows, _, b, _ = ref.bce_rows(p, y, "probs")
        assert (np.abs(ref.bce_rows_fp32(p, y, "probs") - rows) <= b).all()


def test_bce_mutants_leave_the_bound(gold):
    x, y = gold["bce.x"], gold["bce.y"]
    rows, _, b, _ = ref.bce_rows(x, y, "logits")
    with np.errstate(all="ignore"):
        bad = ref.bce_rows_fp32(x, y, "logits", mutant="unstable_log").astype(np.float64)
    print("unstable_log: row 0 is", bad[0], "against", rows[0])
    assert not np.abs(bad[0] - rows[0]) <= b[0]                              # inf - inf at x = 1e4
    p, yp = gold["bce.p"], gold["bce.yp"]
    rows, _, b, _ = ref.bce_rows(p, yp, "probs")
    with np.errstate(all="ignore"):
        bad = ref.bce_rows_fp32(p, yp, "probs", mutant="no_clamp").astype(np.float64)
    print("no_clamp: row 0 is", bad[0], "against", rows[0])
    assert not np.abs(bad[0] - rows[0]) <= b[0]                              # -log(0) where the clamp gives 100


# ---- lookups, config, helpers ----------------------------------------------------------------------------------------------
def test_get_loss_func_config_keys_and_label_helpers():
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.datasets import utils
    from focus_amd.slowfast.models import losses
    cfg = get_cfg()
    assert cfg.DATA.MULTI_LABEL is False and cfg.DATA.ENSEMBLE_METHOD == "sum"
    for name, cls in (("bce", losses.BCELoss), ("bce_logit", losses.BCEWithLogitsLoss)):
        cfg.MODEL.LOSS_FUNC = name
        assert losses.get_loss_func(cfg) is cls and cls(reduction="mean").reduction == "mean" and cls(reduction="sum")
        with pytest.raises(NotImplementedError):
            cls(reduction="none")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls()(torch.rand(2, 3), torch.rand(2, 3))
    cfg.TRAIN.DATASET = "epickitchens"
    with pytest.raises(NotImplementedError, match="epickitchens"):
        losses.get_loss_func(cfg)
    v = utils.as_binary_vector([3, 1, 3], 5)
    assert v.dtype == np.float64 and v.tolist() == [0, 1, 0, 1, 0]
    assert sorted(utils.aggregate_labels([[1, 2], [2, 5], []])) == [1, 2, 5]


def test_new_entry_points_validate_before_launching(built):
    from focus_amd import _lib, ops
    decl = _lib.parse_header()
    for name in ("focus_bce_rows", "focus_view_accumulate_dense", "focus_average_precision", "focus_average_precision_workspace_bytes"):
        assert name in decl
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr, odd = ctypes.c_void_p(a), ctypes.c_void_p(a + 4)
    OK, NULL, SHAPE, DTYPE, ALIGN, WORKSPACE = 0, -5, -1, -2, -3, -6
    assert lib.focus_bce_rows(None, 7, ptr, 7, 2, 7, 0, 1.0, ptr, ptr, 7, None) == NULL
    assert lib.focus_bce_rows(ptr, 7, ptr, 7, 2, 7, 0, 1.0, ptr, None, 7, None) == NULL
    assert lib.focus_bce_rows(ptr, 7, ptr, 7, 2, 0, 0, 1.0, ptr, ptr, 7, None) == SHAPE
    assert lib.focus_bce_rows(ptr, 6, ptr, 7, 2, 7, 0, 1.0, ptr, ptr, 7, None) == SHAPE          # a row stride below C
    assert lib.focus_bce_rows(ptr, 7, ptr, 7, 2, 7, 2, 1.0, ptr, ptr, 7, None) == SHAPE          # an unknown mode
    assert lib.focus_bce_rows(ptr, 7, ptr, 7, -1, 7, 0, 1.0, ptr, ptr, 7, None) == SHAPE
    assert lib.focus_bce_rows(ptr, 7, ptr, 7, 0, 7, 1, 1.0, ptr, ptr, 7, None) == OK             # empty: no launch
    vd = lib.focus_view_accumulate_dense
    assert vd(ptr, 0, 2, 5, 5, ptr, None, 5, 3, 4, 0, ptr, ptr, ptr, ptr, None) == NULL
    assert vd(ptr, 0, 2, 5, 5, ptr, ptr, 5, 0, 4, 0, ptr, ptr, ptr, ptr, None) == SHAPE          # num_clips < 1
    assert vd(ptr, 0, 2, 5, 5, ptr, ptr, 4, 3, 4, 0, ptr, ptr, ptr, ptr, None) == SHAPE          # ldl < C
    assert vd(ptr, 0, 2, 5, 5, ptr, ptr, 5, 3, 4, 2, ptr, ptr, ptr, ptr, None) == SHAPE          # an unknown mode
    assert vd(ptr, 2, 2, 5, 5, ptr, ptr, 5, 3, 4, 0, ptr, ptr, ptr, ptr, None) == DTYPE
    assert vd(ptr, 0, 0, 5, 5, ptr, ptr, 5, 3, 4, 1, ptr, ptr, ptr, ptr, None) == OK
    ws = lib.focus_average_precision_workspace_bytes
    assert ws(1, 1) == 16 and ws(256, 7) == 7 * 16 and ws(257, 7) == 2 * 7 * 16 and ws(0, 7) == 0
    ap = lib.focus_average_precision
    assert ap(ptr, 3, None, 3, 4, 3, ptr, ptr, ptr, ptr, ptr, 64, None) == NULL
    assert ap(ptr, 3, ptr, 3, 4, 0, ptr, ptr, ptr, ptr, ptr, 64, None) == SHAPE
    assert ap(ptr, 2, ptr, 3, 4, 3, ptr, ptr, ptr, ptr, ptr, 64, None) == SHAPE                  # lds < C
    assert ap(ptr, 3, ptr, 3, 4, 70000, ptr, ptr, ptr, ptr, ptr, 64, None) == SHAPE
    assert ap(ptr, 3, ptr, 3, 0, 3, ptr, ptr, ptr, ptr, None, 0, None) == OK                     # empty: no launch
    assert ap(ptr, 3, ptr, 3, 4, 3, ptr, ptr, ptr, ptr, None, 64, None) == NULL
    assert ap(ptr, 3, ptr, 3, 4, 3, ptr, ptr, ptr, ptr, odd, 64, None) == ALIGN
    assert ap(ptr, 3, ptr, 3, 4, 3, ptr, ptr, ptr, ptr, ptr, 47, None) == WORKSPACE
    x = torch.rand(4, 3)
    for call in (lambda: ops.bce_with_logits(x, x), lambda: ops.bce(x, x), lambda: ops.average_precision(x, x),
                 lambda: ops.view_accumulate_dense(x, torch.zeros(4, dtype=torch.long), x, 1, x, x, torch.zeros(4, dtype=torch.long),
                                                   torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- MultiLabelStats -------------------------------------------------------------------------------------------------------
def test_multi_label_stats_on_the_host(gold):
    from focus_amd.slowfast.utils import meters
    s, y = gold["ap.random300.scores"], gold["ap.random300.labels"]
    st = meters.MultiLabelStats("cpu", s.shape[1], 300)
    for a, b in ((0, 100), (100, 101), (101, 300)):
        st.update(torch.from_numpy(s[a:b]), torch.from_numpy(y[a:b]))
    with pytest.raises(RuntimeError, match="do not fit"):
        st.update(torch.from_numpy(s[:1]), torch.from_numpy(y[:1]))
    out = st.read()
    assert out == {"map": float(meters.get_map(s, y)), "samples": 300} and st.offset == 0
    assert abs(out["map"] - float(gold["ap.random300.map"])) <= ref.map_bound(*s.shape)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from focus_amd.slowfast.utils import meters
    g = np.load(os.path.join(ROOT, "tests", "golden", "multilabel.npz"))
    s, y = torch.from_numpy(g["ap.random300.scores"]), torch.from_numpy(g["ap.random300.labels"])
    cut = 180                                                        # uneven parts: rank 0 holds 180 rows, rank 1 holds 120
    lo, hi = (0, cut) if rank == 0 else (cut, 300)
    st = meters.MultiLabelStats("cpu", s.shape[1], 200)
    st.update(s[lo:lo + 50], y[lo:lo + 50])
    st.update(s[lo + 50:hi], y[lo + 50:hi])
    got = st.read()
    ok = got == {"map": float(meters.get_map(s, y)), "samples": 300}
    st.update(s[lo:hi], y[lo:hi])
    ok &= st.read(reduce=False) == {"map": float(meters.get_map(s[lo:hi], y[lo:hi])), "samples": hi - lo}
    with open(out + str(rank), "w") as f:
        f.write("%d" % ok)
    dist.barrier()
    dist.destroy_process_group()


def test_multi_label_stats_two_ranks_gloo(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "res")
    mp.spawn(_gloo_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert open(out + "0").read() == "1" and open(out + "1").read() == "1"
