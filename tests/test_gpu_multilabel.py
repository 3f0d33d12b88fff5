"""GPU: csrc/multilabel.hip against its float64 twin (tests/multilabel_ref.py) and the fixture recorded from the reference
(tests/golden/multilabel.npz), and the multi-label route through the meters and the loops.  focus_bce_rows: rows and
gradient inside the bound derived in the twin, guard elements untouched.  focus_view_accumulate_dense: the tables bit for
bit.  focus_average_precision: npos equal, ap and summary bit-equal to the counting twin (which restates the order of the
sums) and inside the bound against the sorting form, every flag bit, two launches bit-equal."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import multilabel_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from focus_amd import ops
    return ops


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "multilabel.npz")))


def padded(a, pad, fill=777.0):
    """A device view [R,C] into a [R,C+pad] buffer filled with `fill`."""
    a = torch.as_tensor(a)
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=a.dtype, device="cuda")
    buf[:, :a.shape[1]] = a.cuda()
    return buf[:, :a.shape[1]], buf


# ---- focus_bce_rows --------------------------------------------------------------------------------------------------------
def bce_inputs(R, C, mode, seed):
    g = np.random.RandomState(seed)
    y = g.rand(R, C).astype(np.float32)                                       # soft targets
    if mode == "logits":
        x = (g.randn(R, C) * 6).astype(np.float32)
        plant = np.float32([1e4, -1e4, 0.0, 1e4, -1e4])
        yp = np.float32([1.0, 1.0, 0.5, 0.0, 0.0])
    else:
        x = g.rand(R, C).astype(np.float32)
        plant = np.float32([0.0, 1.0, 1e-8, 0.0, 1.0, 1e-8])
        yp = np.float32([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    k = min(plant.size, R * C)
    x.reshape(-1)[:k], y.reshape(-1)[:k] = plant[:k], yp[:k]
    if R * C > 40:                                                            # the planted values with another target, at the end
        n = min(6, plant.size)
        x.reshape(-1)[R * C - 6:R * C - 6 + n], y.reshape(-1)[R * C - 6:R * C - 6 + n] = plant[:n], 0.25
    return x, y


@pytest.mark.parametrize("mode", ["logits", "probs"])
@pytest.mark.parametrize("R", [1, 3, 65])
def test_bce_rows_and_gradient_inside_the_bound_guards_untouched(ops, mode, R):
    from focus_amd import _lib
    worst = [0.0, 0.0]
    for C in (1, 7, 157, 257, 1000):
        x, y = bce_inputs(R, C, mode, 100 * R + C)
        gs = 1.0 / (R * C)
        xv, xb = padded(x, 3)
        yv, yb = padded(y, 5)
        dv, db = padded(np.zeros_like(x), 2, fill=-555.0)
        db.fill_(-555.0)
        rows_d = torch.full((R + 1,), -555.0, device="cuda")
        _lib.check(_lib.lib().focus_bce_rows(ops._p(xv), xb.stride(0), ops._p(yv), yb.stride(0), R, C, ops.BCE_MODES[mode], gs,
                                             ops._p(rows_d), ops._p(dv), db.stride(0), ops._stream()), "bce_rows")
        rows, dx, row_b, dx_b = ref.bce_rows(x, y, mode, gs)
        got_r, got_d = rows_d[:R].cpu().double().numpy(), dv.cpu().double().numpy()
        assert np.isfinite(got_r).all() and np.isfinite(got_d).all()
        worst = [max(worst[0], (np.abs(got_r - rows) / row_b).max()), max(worst[1], (np.abs(got_d - dx) / dx_b).max())]
        assert (np.abs(got_r - rows) <= row_b).all(), (C, np.abs(got_r - rows) / row_b)
        assert (np.abs(got_d - dx) <= dx_b).all(), (C, (np.abs(got_d - dx) / dx_b).max())
        assert float(rows_d[R]) == -555.0 and bool((db[:, C:] == -555.0).all())
        assert bool((xb[:, C:] == 777.0).all()) and bool((yb[:, C:] == 777.0).all())
    print(mode, "R", R, "worst row error / bound %.3g, dx %.3g" % tuple(worst))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bce_operators_value_and_gradient_against_the_twin(ops, reduction, dtype):
    for mode, fn, (R, C) in (("logits", ops.bce_with_logits, (8, 157)), ("probs", ops.bce, (3, 7)), ("logits", ops.bce_with_logits, (1, 1))):
        x, y = bce_inputs(R, C, mode, 9)
        xt = torch.from_numpy(x).cuda().to(dtype)
        x = xt.float().cpu().numpy()                                          # what the kernel sees after the widening
        xt.requires_grad_(True)
        yv, _ = padded(y, 4)
        loss = fn(xt, yv, reduction)
        (3.0 * loss).backward()
        gs = 1.0 / (R * C) if reduction == "mean" else 1.0
        rows, dx, row_b, dx_b = ref.bce_rows(x, y, mode, gs)
        assert loss.dtype == torch.float32 and abs(float(loss.detach()) - rows.sum() * gs) <= ref.loss_bound(rows, row_b, gs)
        got = xt.grad.double().cpu().numpy()
        b = 3.0 * dx_b + ref.U32 * np.abs(3.0 * dx)                                  # the product with the incoming gradient
        if dtype == torch.bfloat16:
            b = b + 2.0 ** -8 * (np.abs(3.0 * dx) + b)                               # one rounding to bf16: 8 significant bits
        assert xt.grad.dtype == dtype and (np.abs(got - 3.0 * dx) <= b).all()
        assert not yv.requires_grad


def test_bce_operators_equal_torch_within_the_bound_and_refuse(ops, gold):
    x, y = gold["bce.x"], gold["bce.y"]
    loss = ops.bce_with_logits(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), "mean")
    rows, _, row_b, _ = ref.bce_rows(x, y, "logits")
    assert abs(float(loss) - float(gold["bce.logit.f64.mean"])) <= ref.loss_bound(rows, row_b, 1.0 / x.size)
    p, yp = gold["bce.p"], gold["bce.yp"]
    loss = ops.bce(torch.from_numpy(p).cuda(), torch.from_numpy(yp).cuda(), "sum")
    rows, _, row_b, _ = ref.bce_rows(p, yp, "probs")
    assert abs(float(loss) - float(gold["bce.prob.f64.sum"])) <= ref.loss_bound(rows, row_b, 1.0)
    t = torch.rand(2, 3, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.bce_with_logits(t, t, "none")
    with pytest.raises(ValueError):
        ops.bce(t, t[:, :2], "mean")
    with pytest.raises(ValueError):
        ops.bce_with_logits(t[0], t[0], "mean")


# ---- focus_view_accumulate_dense -------------------------------------------------------------------------------------------
def dense_tables(NV, C):
    return (torch.full((NV, C), -1e10, device="cuda"), torch.zeros(NV, C, device="cuda"),
            torch.zeros(NV, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("mode", ["max", "sum"])
def test_dense_view_fold_equals_the_fixture_and_the_twin_bit_for_bit(ops, gold, mode):
    t = {k: gold["tm.%s.%s" % (mode, k)] for k in ("preds", "labels", "clip_ids", "splits", "video_preds", "video_labels", "clip_count")}
    NV, C = t["video_preds"].shape
    vp, vl, cc, flag = dense_tables(NV, C)
    o = 0
    for n in t["splits"]:                                                    # videos' clips are split over the calls
        sl = slice(o, o + n)
        pv, _ = padded(t["preds"][sl], 3)
        lv, _ = padded(t["labels"][sl], 1)
        ops.view_accumulate_dense(pv, torch.from_numpy(t["clip_ids"][sl]).cuda(), lv, 3, vp, vl, cc, flag, mode)
        o += n
    assert np.array_equal(vp.cpu().numpy().view(np.uint32), t["video_preds"].view(np.uint32))
    assert np.array_equal(vl.cpu().numpy(), t["video_labels"]) and np.array_equal(cc.cpu().numpy(), t["clip_count"])
    assert int(flag) == 0
    if mode == "sum":
        assert bool((vp == -1e10).all())                                      # the reference's arithmetic: every score is swallowed


@pytest.mark.parametrize("mode,dtype,C", [("sum", torch.float32, 300), ("max", torch.bfloat16, 300), ("max", torch.float32, 1),
                                          ("sum", torch.bfloat16, 257)])
def test_dense_view_fold_wide_rows_from_zero_tables(ops, mode, dtype, C):
    g = np.random.RandomState(C)
    NV, NC = 5, 4
    preds = torch.from_numpy(g.randn(NV * NC, C).astype(np.float32)).to(dtype)
    vlab = (g.rand(NV, C) < 0.3).astype(np.float32)
    vlab[:, 0] = 1
    ids = g.permutation(NV * NC).astype(np.int64)
    ids[3] = NV * NC + 2                                                      # out of range: skipped, bit 1
    ids[9] = -1
    labels = vlab[np.clip(ids, 0, NV * NC - 1) // NC]
    vp, vl, cc, flag = (torch.zeros(NV, C, device="cuda"), torch.zeros(NV, C, device="cuda"),
                        torch.zeros(NV, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    wp, wl, wc, wf = np.zeros((NV, C), np.float32), np.zeros((NV, C), np.float32), np.zeros(NV, np.int64), np.zeros(1, np.int32)
    for a, b in ((0, 7), (7, 8), (8, 20)):
        pv, _ = padded(preds[a:b], 5)
        lv, _ = padded(labels[a:b], 2)
        ops.view_accumulate_dense(pv, torch.from_numpy(ids[a:b]).cuda(), lv, NC, vp, vl, cc, flag, mode)
        ref.view_accumulate_dense(preds[a:b].float().numpy(), ids[a:b], labels[a:b], NC, wp, wl, wc, wf, mode)
    assert np.array_equal(vp.cpu().numpy().view(np.uint32), wp.view(np.uint32))
    assert np.array_equal(vl.cpu().numpy(), wl) and np.array_equal(cc.cpu().numpy(), wc) and int(flag) == wf[0] == 2


def test_dense_view_fold_flags_a_contradicting_row_and_writes_it(ops):
    vp, vl, cc, flag = dense_tables(2, 3)
    p = torch.tensor([[1., 2, 3], [3, 2, 1]], device="cuda")
    ops.view_accumulate_dense(p, torch.tensor([0, 1], device="cuda"), torch.tensor([[1., 0, 0], [1, 0, 0]], device="cuda"), 2, vp, vl,
                              cc, flag, "max")
    assert int(flag) == 0 and vp[0].tolist() == [3, 2, 3] and bool((vp[1] == -1e10).all()) and cc.tolist() == [2, 0]
    ops.view_accumulate_dense(p, torch.tensor([2, 3], device="cuda"), torch.tensor([[0., 0, 0], [0, 1, 0]], device="cuda"), 2, vp, vl,
                              cc, flag, "max")
    assert int(flag) == 0 and vl[1].tolist() == [0, 1, 0]                     # an all-zero stored row is "not seen yet"
    ops.view_accumulate_dense(p[:1], torch.tensor([1], device="cuda"), torch.tensor([[0., 1, 0]], device="cuda"), 2, vp, vl, cc, flag, "max")
    assert int(flag) == 1 and vl[0].tolist() == [0, 1, 0] and cc.tolist() == [3, 2]
    ops.view_accumulate_dense(p[:1], torch.tensor([4], device="cuda"), torch.tensor([[0., 1, 0]], device="cuda"), 2, vp, vl, cc, flag, "max")
    assert int(flag) == 3                                                     # sticky


# ---- focus_average_precision -----------------------------------------------------------------------------------------------
def ap_table(N, C, seed):
    """Columns by c % 5: scores quantised to three values; all scores equal; every row a positive; no positive; normal scores
    with a block of rows still at -1e10."""
    g = np.random.RandomState(seed)
    s = g.randn(N, C).astype(np.float32)
    y = (g.rand(N, C) < 0.3).astype(np.float32)
    for c in range(C):
        k = c % 5
        if k == 0:
            s[:, c] = g.choice(np.float32([-1.5, 0.25, 3.0]), size=N)
        elif k == 1:
            s[:, c] = 0.5
        elif k == 2:
            y[:, c] = 1
        elif k == 3:
            y[:, c] = 0
        else:
            s[g.rand(N) < 0.2, c] = -1e10
    return s, y


@pytest.fixture(scope="module")
def ap_twins():
    """The twin's results, computed once per shape."""
    out = {}
    for N in (1, 2, 63, 64, 65, 257, 1000):
        for C in (1, 7, 33):
            s, y = ap_table(N, C, 1000 * C + N)
            out[N, C] = (s, y) + ref.average_precision_counting(s, y)
    return out


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000])
def test_average_precision_equals_the_twin(ops, ap_twins, N):
    for C in (1, 7, 33):
        s, y, ap, npos, summary, flag = ap_twins[N, C]
        sv, _ = padded(s, 3)                                                  # a row stride wider than C
        yv, _ = padded(y, 0 if C == 7 else 6)
        g_ap, g_npos, g_sum, g_flag = ops.average_precision(sv, yv)
        again = ops.average_precision(sv, yv)
        assert all(torch.equal(a, b) for a, b in zip((g_ap, g_npos, g_sum, g_flag), again))       # the same bits twice
        assert g_ap.dtype == torch.float64 and g_npos.dtype == torch.int64 and g_sum.shape == (2,) and g_flag.dtype == torch.int32
        assert np.array_equal(g_npos.cpu().numpy(), npos) and int(g_flag) == flag
        got = g_ap.cpu().numpy()
        kept = npos > 0
        sort = np.array([ref.average_precision_sorting(s[:, c], y[:, c]) if kept[c] else 0.0 for c in range(C)])
        d = np.abs(got - sort).max()
        print("N", N, "C", C, "kernel - sorting form %.3g, bound %.3g" % (d, ref.ap_bound(N)), "bit-equal to the counting twin:",
              np.array_equal(got, ap))
        assert d <= ref.ap_bound(N)
        assert np.array_equal(got, ap) and np.array_equal(g_sum.cpu().numpy(), summary)          # the twin restates the order
        assert not got[~kept].any() and g_sum[1] == kept.sum()


def test_average_precision_equals_the_recorded_reference(ops, gold):
    from focus_amd.slowfast.utils import meters
    for case in ("ties", "zero_class", "one_class", "single_kept", "fill", "nan", "none_kept", "random300", "all_equal"):
        s, y, want = gold["ap.%s.scores" % case], gold["ap.%s.labels" % case], float(gold["ap.%s.map" % case])
        got = meters.get_map(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda())
        print(case, "device get_map - reference %.3g" % (float(got) - want))
        assert abs(float(got) - want) <= ref.map_bound(*s.shape)
        if "ap.%s.aps" % case in gold:
            ap, npos, _, _ = ops.average_precision(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda())
            assert np.abs(ap.cpu().numpy()[npos.cpu().numpy() > 0] - gold["ap.%s.aps" % case]).max() <= ref.ap_bound(s.shape[0])


def test_average_precision_flag_bits(ops):
    from focus_amd.slowfast.utils import meters
    s, y = ap_table(300, 7, 3)
    flag_of = lambda a, b: int(ops.average_precision(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())[3])
    assert flag_of(s, y) == 0
    b = y.copy()
    b[299, 0] = 0.5                                                           # a kept class, the second tile
    assert flag_of(s, b) == ops.AP_BAD_LABEL
    with pytest.raises(ValueError, match="0 or 1"):
        meters.get_map(torch.from_numpy(s).cuda(), torch.from_numpy(b).cuda())
    for bad in (np.nan, np.inf, -np.inf):
        a = s.copy()
        a[7, 3] = bad                                                         # column 3 has no positive: dropped with its score
        assert flag_of(a, y) == 0
        a[280, 4] = bad
        assert flag_of(a, y) == ops.AP_BAD_SCORE
        assert meters.get_map(torch.from_numpy(a).cuda(), torch.from_numpy(y).cuda()) == 0.0
    b[299, 0], b[5, 2] = 2.0, np.nan
    a[280, 4] = np.nan
    assert flag_of(a, b) == ops.AP_BAD_LABEL | ops.AP_BAD_SCORE
    ap, npos, summary, flag = ops.average_precision(torch.from_numpy(s).cuda(), torch.zeros(300, 7, device="cuda"))
    assert int(flag) == ops.AP_NO_CLASS and not ap.any() and not npos.any() and summary.tolist() == [0.0, 0.0]
    ap, npos, summary, flag = ops.average_precision(torch.zeros(0, 4, device="cuda"), torch.zeros(0, 4, device="cuda"))
    assert int(flag) == ops.AP_NO_CLASS and ap.shape == (4,) and summary.tolist() == [0.0, 0.0]
    t = torch.rand(4, 3, device="cuda")
    for a, b in ((t, t.long()), (t, t[:, :2]), (t.t(), t.t()), (t[0], t[0])):
        with pytest.raises(ValueError):
            ops.average_precision(a, b)


# ---- the meters and the loops ----------------------------------------------------------------------------------------------
class Scores(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, inputs, meta):
        return inputs[0].flatten(1)[:, :9] + self.w


@pytest.mark.parametrize("method", ["max", "sum"])
def test_perform_test_device_meter_equals_the_host_meter(method):
    from focus_amd.slowfast.utils import meters
    from focus_amd.train import perform_test
    V, NC, C = 7, 3, 9
    g = torch.Generator().manual_seed(5)
    clips = torch.rand(V * NC, 20, generator=g)
    vlab = (torch.rand(V, C, generator=g) < 0.4).float()
    vlab[:, 1] = 1 - vlab[:, 0]                                               # every video has a label
    ids = torch.randperm(V * NC, generator=g)
    loader = [([clips[ids[i:i + 4]]], vlab[ids[i:i + 4] // NC], ids[i:i + 4], {}) for i in range(0, V * NC, 4)]
    dev = meters.DeviceTestMeter(V, NC, C, len(loader), "cuda", ensemble_method=method, multi_label=True)
    host = meters.TestMeter(V, NC, C, len(loader), multi_label=True, ensemble_method=method)
    sd, sh = perform_test(loader, Scores().cuda(), dev, None), perform_test(loader, Scores().cuda(), host, None)
    assert dev.video_preds.is_cuda and torch.equal(dev.video_preds.cpu(), host.video_preds)
    assert torch.equal(dev.video_labels.cpu(), host.video_labels) and torch.equal(dev.clip_count.cpu(), host.clip_count)
    assert set(sd) == set(sh) == {"split", "complete", "map"} and sd["complete"] and sh["complete"]
    assert abs(float(sd["map"]) - float(sh["map"])) <= ref.map_bound(V, C) and 0 < float(sd["map"]) <= 1
    dev.update_stats(clips[:1, :9].cuda(), 1 - vlab[:1], torch.zeros(1, dtype=torch.long))       # contradicts video 0
    with pytest.raises(AssertionError, match="clips of one video disagree"):
        dev.finalize_metrics()
    dev.reset()
    assert bool((dev.video_preds == -1e10).all()) and not dev.video_labels.any() and int(dev.flag) == 0
    assert dev.finalize_metrics() == {"split": "test_final", "complete": False, "map": 0.0}


def test_eval_epoch_multi_label_returns_the_map_of_all_batches():
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.utils import meters
    from focus_amd.train import eval_epoch
    g = torch.Generator().manual_seed(7)
    clips = torch.rand(10, 20, generator=g)
    labels = (torch.rand(10, 9, generator=g) < 0.4).float()
    cfg = get_cfg()
    cfg.merge_from_list(["DATA.MULTI_LABEL", True, "MODEL.LOSS_FUNC", "bce_logit", "DATA.ENSEMBLE_METHOD", "max"])
    loader = [([clips[i:i + 4]], labels[i:i + 4], None, {}) for i in range(0, 10, 4)]
    m = Scores().cuda().train()
    e = eval_epoch(loader, m, cfg)
    want = float(meters.get_map(clips[:, :9].numpy(), labels.numpy()))
    assert not m.training and set(e) == {"map", "samples"} and e["samples"] == 10
    assert abs(e["map"] - want) <= ref.map_bound(10, 9) and want > 0
    st = meters.MultiLabelStats("cuda", 9, 8)
    st.update(clips[:8, :9].cuda(), labels[:8])
    with pytest.raises(RuntimeError, match="do not fit"):
        st.update(clips[:1, :9].cuda(), labels[:1])
    assert eval_epoch(loader[:2], m, cfg, stats=meters.MultiLabelStats("cuda", 9, 8))["samples"] == 8


def test_train_iter_multi_label_step_keeps_the_loss_and_no_topk_without_a_sync():
    from focus_amd import train
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import build_model
    from focus_amd.slowfast.models.losses import BCEWithLogitsLoss, get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    from focus_amd.slowfast.utils import meters
    cfg = get_cfg()
    cfg.merge_from_list(["ORVIT.ENABLE", True, "ORVIT.O", 3, "ORVIT.LAYERS", [1], "DATA.TRAIN_CROP_SIZE", 64,
                         "DATA.NUM_FRAMES", 4, "MF.EMBED_DIM", 64, "MF.DEPTH", 3, "MF.NUM_HEADS", 4,
                         "MF.TEMPORAL_RESOLUTION", 2, "MF.USE_MLP", True, "MODEL.NUM_CLASSES", 10,
                         "MODEL.MODEL_NAME", "Motionformer", "TRAIN.DATASET", "Ssv2", "NUM_GPUS", 1,
                         "TRAIN.MIXED_PRECISION", False, "MODEL.LOSS_FUNC", "bce_logit", "DATA.MULTI_LABEL", True,
                         "DATA.ENSEMBLE_METHOD", "max", "SOLVER.OPTIMIZING_METHOD", "adamw", "SOLVER.BASE_LR", 1e-3,
                         "SOLVER.CLIP_GRAD_L2NORM", 1.0])
    torch.manual_seed(0)
    m = build_model(cfg).train()
    opt = construct_optimizer(m, cfg)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    assert isinstance(loss_fun, BCEWithLogitsLoss)
    inputs, _, meta = train.synthetic_batch(cfg, 2, "cuda")
    labels = torch.tensor([[1., 0, 0, 1, 0, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0, 0, 0, 0, 0]], device="cuda")
    stats = meters.StepStats("cuda")
    before = [p.detach().clone() for p in m.parameters()]
    train.train_iter(m, opt, loss_fun, inputs, labels, meta, cfg, stats=stats)                   # warm-up: lazy set-up may sync
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        preds, out_labels, loss = train.train_iter(m, opt, loss_fun, inputs, labels, meta, cfg, stats=stats)
    names = {e.name for e in prof.events()}
    assert "aten::item" not in names and "aten::_local_scalar_dense" not in names
    assert out_labels is labels and preds.shape == (2, 10)
    x = preds.detach().double().cpu().numpy()
    want = np.mean(np.maximum(x, 0) - x * labels.cpu().numpy() + np.log1p(np.exp(-np.abs(x))))
    assert np.isfinite(float(loss.detach())) and abs(float(loss.detach()) - want) < 1e-5
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
    assert int(stats.acc_i[4:].sum()) == 0                                    # the top-k columns stay zero
    w = stats.read()
    assert w["steps"] == 2 and w["samples"] == 4 and np.isfinite(w["loss"]) and w["top1_err"] == 100.0
