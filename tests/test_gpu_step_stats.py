"""csrc/step_stats.hip on the device: focus_topk_stats against the numpy twin (tests/step_stats_ref.py) with counts equal as
integers, its accumulation over launches with the loss sums bit-equal to the host's double sums, focus_view_accumulate bit
for bit against the twin and the reference-order per-clip loop, the meters and loops built on the two (StepStats,
DeviceTestMeter, EPICTestMeter, train_iter / slot_train_step's stats=, eval_epoch, the EK branch of perform_test), and the
refusals of the operators.

Shapes: the class counts straddle the 64 lanes of the wave that owns a row (5, 6, 63, 64, 65, ... 300: one to five trips of
its loop, with and without a partial trip), the batches straddle the four rows of a workgroup (1, 3, 8: a partial
workgroup, and two of them)."""
import numpy as np
import pytest
import torch

import mixup_ref
import step_stats_ref as ref

pytestmark = pytest.mark.gpu

VS = (5, 6, 63, 64, 65, 97, 174, 255, 256, 257, 300)
BS = (1, 3, 8)
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def ops():
    from focus_amd import ops
    return ops


def dev_logits(rows, dtype, pad):
    t = torch.from_numpy(rows).cuda().to(dtype)
    if pad:                                                    # a column slice of a wider tensor: row stride V + pad, odd offset
        wide = torch.full((t.shape[0], t.shape[1] + pad), 3.0e38, device="cuda", dtype=dtype)
        wide[:, 3:3 + t.shape[1]] = t
        t = wide[:, 3:3 + t.shape[1]]
        assert not t.is_contiguous() or t.shape[0] == 1
    return t


def dev_labels(l, pad=0):
    l = np.asarray(l)
    if l.ndim == 1:
        return torch.from_numpy(l.astype(np.int64)).cuda()
    t = torch.from_numpy(l.astype(np.float32)).cuda()
    if pad:
        wide = torch.full((t.shape[0], t.shape[1] + pad), 2.0, device="cuda")
        wide[:, 2:2 + t.shape[1]] = t
        t = wide[:, 2:2 + t.shape[1]]
    return t


def both(ops, preds, labels, ks, dtype, pad=0):
    """(kernel, twin) accumulators after one batch."""
    acc_i = torch.zeros(16, dtype=torch.int64, device="cuda")
    acc_f = torch.zeros(8, dtype=torch.float64, device="cuda")
    ops.topk_stats(acc_i, acc_f, tuple(dev_logits(p, dtype, pad) for p in preds), tuple(dev_labels(l, pad) for l in labels), ks)
    want = ref.new_acc()
    ref.topk_stats(*want, preds, labels, ks, bf16=dtype == torch.bfloat16)
    return acc_i.cpu().numpy(), want[0]


def tied_rows(B, V, seed, nans=0):
    """Rows of few distinct (bf16-exact) values, so that ties are everywhere; `nans` entries per row are NaN."""
    g = np.random.RandomState(seed)
    rows = (np.round(g.randn(B, V) * 2) / 2).astype(np.float32)
    for r in range(B):
        rows[r, g.randint(0, V, nans)] = np.nan
    return rows


def tied_dense(B, V, seed):
    g = np.random.RandomState(seed)
    return (np.round(g.rand(B, V) * 4) / 4).astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_counts_equal_the_twin_on_every_shape(ops, dtype):
    for V in VS:
        for B in BS:
            g = np.random.RandomState(V * 31 + B)
            rows = ref.tie_free_rows(B, V, seed=V * 10 + B)
            l = g.randint(0, V, B)
            dense = mixup_ref.target(l, V, 0.3, 0.1)
            for labels in (l, dense):
                for pad in (0, 7):
                    got, want = both(ops, (rows,), (labels,), (1, 5), dtype, pad)
                    assert np.array_equal(got, want), (V, B, labels.ndim, pad, got, want)
            ties = tied_rows(B, V, seed=V + B, nans=0)
            for labels in (l, tied_dense(B, V, seed=V * 7 + B)):
                got, want = both(ops, (ties,), (labels,), (1, 5), dtype, 7)
                assert np.array_equal(got, want), ("ties", V, B, labels.ndim, got, want)
            assert want[ref.CORRECT + 1] >= want[ref.CORRECT]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ks", [(1, 5), (1,), (1, 2, 3, 5)])
def test_two_heads_ks_ties_and_nans(ops, dtype, ks):
    for (V0, V1) in ((97, 300), (5, 6)):
        for B in BS:
            g = np.random.RandomState(V1 + B)
            l0, l1 = g.randint(0, V0, B), g.randint(0, V1, B)
            for make in (lambda V, s: ref.tie_free_rows(B, V, s), lambda V, s: tied_rows(B, V, s, nans=2)):
                p0, p1 = make(V0, 3 * B), make(V1, 3 * B + 1)
                for labels in ((l0, l1), (mixup_ref.target(l0, V0, 0.8, 0.1), mixup_ref.target(l1, V1, 0.8, 0.1)),
                               (tied_dense(B, V0, B), tied_dense(B, V1, B + 1))):
                    for pad in (0, 7):
                        got, want = both(ops, (p0, p1), labels, ks, dtype, pad)
                        assert np.array_equal(got, want), (V0, V1, B, pad, got, want)
                    one, want1 = both(ops, (p0,), labels[:1], ks, dtype)
                    assert np.array_equal(one, want1) and np.array_equal(one[4:8], one[12:16])   # one head: "every head" = head 0
    # the hand-derived rows of the CPU test, on the device
    nan = float("nan")
    for pred, label, rank in (([1, 2, 2, 0], 2, 1), ([1, 2, 2, 0], 1, 0), ([nan, 3, 1, 0], 1, 1), ([nan, nan, 1, 0], 1, 0),
                              ([nan, nan, 1, 0], 2, 2), ([1, 2, 3, 4], 7, 9)):
        got, want = both(ops, (np.float32([pred]),), ([label],), (1, 2, 3), dtype)
        assert np.array_equal(got, want) and got[4:7].tolist() == [int(rank < k) for k in (1, 2, 3)], (pred, label)
    lab = np.float32([[0, 0.2, 0.7, 0.1]])
    got, want = both(ops, (np.float32([[1.0, 2.0 ** -8, 1.0, -3]]),), (lab,), (1,), dtype)    # the single rounding of the sum
    assert np.array_equal(got, want) and got[4] == (0 if dtype == torch.bfloat16 else 1)
    got, want = both(ops, (ref.tie_free_rows(3, 5, 0),), ([0, 4, 2],), (5,), dtype)           # k = V
    assert np.array_equal(got, want) and got[4] == 3


def test_launches_accumulate_and_the_scalars_follow_the_host(ops):
    acc_i = torch.zeros(16, dtype=torch.int64, device="cuda")
    acc_f = torch.zeros(8, dtype=torch.float64, device="cuda")
    want = ref.new_acc()
    losses = np.float32([[0.1, 1.7, 0.3], [float("inf"), 0.2, 3.0e-7], [float("nan"), 5.0, 1.0], [0.7, 0.9, 2.5],
                         [float("nan"), 0.1, 0.1]])
    host = np.zeros(6, dtype=np.float64)
    for s, (B, V) in enumerate(((3, 97), (8, 97), (5, 97), (1, 97), (2, 97))):
        rows, l = ref.tie_free_rows(B, V, s), np.random.RandomState(s).randint(0, V, B)
        dl = [torch.tensor(float(x), dtype=torch.float32, device="cuda") for x in losses[s]]
        ops.topk_stats(acc_i, acc_f, dev_logits(rows, torch.float32, 0), dev_labels(l), (1, 5), dl)
        ref.topk_stats(*want, (rows,), (l,), (1, 5), losses[s])
        for i in range(3):
            host[i] = host[i] + np.float64(losses[s][i])
            host[3 + i] = host[3 + i] + np.float64(losses[s][i]) * np.float64(B)
    gi, gf = acc_i.cpu().numpy(), acc_f.cpu().numpy()
    assert np.array_equal(gi, want[0]) and gi[:4].tolist() == [5, 19, 1, 2]              # the first NaN step, and it stays
    assert np.array_equal(gf.view(np.uint64), want[1].view(np.uint64))
    assert np.array_equal(gf[[1, 2, 4, 5]].view(np.uint64), host[[1, 2, 4, 5]].view(np.uint64)) and np.isnan(gf[0])
    # no heads (STEVE): only the scalars move; a NULL loss is left alone
    ops.topk_stats(acc_i, acc_f, losses=[torch.tensor(0.5, device="cuda")], batch=6)
    ref.topk_stats(*want, losses=[np.float32(0.5)], batch=6)
    assert np.array_equal(acc_i.cpu().numpy(), want[0]) and acc_i[1] == 25
    assert np.array_equal(acc_f.cpu().numpy()[1:3].view(np.uint64), host[1:3].view(np.uint64))


# ---- focus_view_accumulate ---------------------------------------------------------------------------------------------------
def dev_tables(NV, C):
    return (torch.zeros(NV, C, device="cuda"), torch.zeros(NV, dtype=torch.int64, device="cuda"),
            torch.zeros(NV, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))


def run_views(ops, preds, ids, labels, NC, NV, chunk, mode, dtype, pad=0):
    """The stream of batches through the kernel and the twin -> (device tables as numpy + flag, twin tables + flag)."""
    C = preds.shape[1]
    d = dev_tables(NV, C)
    t = (np.zeros((NV, C), np.float32), np.zeros(NV, np.int64), np.zeros(NV, np.int64))
    flag = 0
    for s in range(0, len(ids), chunk):
        sl = slice(s, s + chunk)
        ops.view_accumulate(dev_logits(preds[sl], dtype, pad), torch.from_numpy(ids[sl]).cuda(), torch.from_numpy(labels[sl]).cuda(),
                            NC, *d, mode=mode)
        flag |= ref.view_accumulate(preds[sl], ids[sl], labels[sl], NC, *t, mode=mode)
    return [x.cpu().numpy() for x in d[:3]] + [int(d[3])], list(t) + [flag]


@pytest.mark.parametrize("V,NC,C,chunk,dtype,mode", [(7, 6, 13, 11, torch.float32, "sum"), (7, 6, 13, 11, torch.float32, "max"),
                                                     (5, 3, 300, 4, torch.bfloat16, "sum"), (5, 3, 97, 15, torch.bfloat16, "sum"),
                                                     (3, 4, 257, 5, torch.float32, "max")])
def test_view_accumulate_is_the_per_clip_loop_bit_for_bit(ops, V, NC, C, chunk, dtype, mode):
    g = torch.Generator().manual_seed(3)
    preds = (torch.rand(V * NC, C, generator=g) * 8 - 2).to(dtype).float().numpy()
    labels_v = torch.randint(1, C, (V,), generator=g).numpy()
    ids = torch.randperm(V * NC, generator=g).numpy()
    for pad in (0, 7):
        got, want = run_views(ops, preds[ids], ids, labels_v[ids // NC], NC, V, chunk, mode, dtype, pad)
        loop = torch.zeros(V, C)                                             # meters.py:316-330 in the order of arrival
        for i in ids:
            p = torch.from_numpy(preds[i])
            loop[i // NC] = loop[i // NC] + p if mode == "sum" else torch.max(loop[i // NC], p)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[0].view(np.uint32), loop.numpy().view(np.uint32))
        assert np.array_equal(got[1], labels_v) and np.array_equal(got[2], np.full(V, NC)) and got[3] == want[3] == 0
    whole, _ = run_views(ops, preds[ids], ids, labels_v[ids // NC], NC, V, V * NC, mode, dtype)     # any split: the same bits
    assert np.array_equal(whole[0].view(np.uint32), got[0].view(np.uint32))


def test_view_accumulate_flags(ops):
    preds = np.float32([[1, 5], [1e8, 2], [-1e8, 7], [3, 3], [float("nan"), 1]])
    ids, labels = np.array([2, 3, 2, 0, 9]), np.array([4, 4, 5, 1, 1])
    got, want = run_views(ops, preds, ids, labels, 2, 2, 5, "sum", torch.float32)
    assert got[3] == want[3] == 3                                            # video 1's clips disagree; id 9 is out of range
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    assert got[0].tolist() == [[3, 3], [0, 14]] and got[1].tolist() == [1, 5] and got[2].tolist() == [1, 3]
    got, want = run_views(ops, preds, np.array([0, 1, 0, 1, 0]), np.array([0, 0, 3, 3, 3]), 2, 1, 2, "max", torch.float32)
    assert got[3] == want[3] == 0 and np.isnan(got[0][0, 0]) and got[0][0, 1] == 7    # a zero label is no label; a NaN stays
    assert np.array_equal(got[0], want[0], equal_nan=True)


# ---- the meters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["sum", "max"])
def test_device_test_meter_equals_test_meter(method):
    from focus_amd.slowfast.utils import meters
    g = torch.Generator().manual_seed(3)
    V, NC, C = 7, 6, 13
    preds = torch.rand(V * NC, C, generator=g)
    labels_v = torch.randint(1, C, (V,), generator=g)
    clip_ids = torch.randperm(V * NC, generator=g)
    host = meters.TestMeter(V, NC, C, 4, ensemble_method=method)
    dev = meters.DeviceTestMeter(V, NC, C, 4, "cuda", ensemble_method=method)
    for n, chunk in enumerate(clip_ids.split(11)):
        host.update_stats(preds[chunk], labels_v[chunk // NC], chunk)
        dev.update_stats(preds[chunk].cuda(), labels_v[chunk // NC] if n % 2 else labels_v[chunk // NC].cuda(), chunk)
    assert torch.allclose(dev.video_preds.cpu(), host.video_preds, atol=1e-6) and torch.equal(dev.video_labels.cpu(), host.video_labels)
    assert dev.finalize_metrics(ks=(1, 5)) == host.finalize_metrics(ks=(1, 5)) and dev.stats["complete"]
    dev.update_stats(preds[:1].cuda(), labels_v[:1] + 1, torch.zeros(1, dtype=torch.long))         # contradicts video 0
    with pytest.raises(AssertionError, match="clips of one video disagree on its label"):
        dev.finalize_metrics()
    dev.reset()
    assert not dev.video_preds.any() and not dev.clip_count.any() and int(dev.flag) == 0
    assert not dev.finalize_metrics()["complete"]


def test_epic_test_meter_agrees_with_the_metrics_of_the_summed_tables():
    from focus_amd.slowfast.utils import meters, metrics
    g = torch.Generator().manual_seed(5)
    V, NC = 6, 3
    verb, noun = torch.rand(V * NC, 97, generator=g), torch.rand(V * NC, 300, generator=g)
    lv, ln = torch.randint(1, 97, (V,), generator=g), torch.randint(1, 300, (V,), generator=g)
    verb[torch.arange(V * NC), lv.repeat_interleave(NC)] += 0.9               # some videos right, some wrong
    noun[torch.arange(V * NC)[::2], ln.repeat_interleave(NC)[::2]] += 0.9
    names = ["P01_%d" % i for i in range(V * NC)]
    ids = torch.randperm(V * NC, generator=g)
    m = meters.EPICTestMeter(V, NC, (97, 300), 3, "cuda")
    for chunk in ids.split(7):
        m.update_stats((verb[chunk].cuda(), noun[chunk].cuda()), (lv[chunk // NC], ln[chunk // NC]),
                       {"narration_id": [names[i] for i in chunk.tolist()]}, chunk)
    (pv, pn), (gv, gn), meta = m.finalize_metrics(ks=(1, 5))
    sv, sn = torch.zeros(V, 97), torch.zeros(V, 300)
    for i in ids.tolist():
        sv[i // NC] += verb[i]
        sn[i // NC] += noun[i]
    assert np.array_equal(pv, sv.numpy()) and np.array_equal(pn, sn.numpy()) and np.array_equal(gv, lv.numpy()) and np.array_equal(gn, ln.numpy())
    assert all(meta[v] in names[v * NC:(v + 1) * NC] for v in range(V)) and bool((m.clip_count == NC).all())
    want = {"split": "test_final"}
    for name, acc in (("verb", metrics.topk_accuracies(sv, lv, (1, 5))), ("noun", metrics.topk_accuracies(sn, ln, (1, 5))),
                      ("action", metrics.multitask_topk_accuracies((sv, sn), (lv, ln), (1, 5)))):
        for k, a in zip((1, 5), acc):
            want["%s_top%d_acc" % (name, k)] = "{:.{prec}f}".format(a, prec=2)
    assert m.stats == want


# ---- the loops -------------------------------------------------------------------------------------------------------------
class Small(torch.nn.Module):
    def __init__(self, V=174):
        super().__init__()
        self.a, self.b = torch.nn.Linear(3 * 2 * 8 * 8, 32), torch.nn.Linear(32, V)

    def forward(self, inputs, meta=None):
        return self.b(torch.tanh(self.a(inputs[0].flatten(1))))


def _loop(mix, use_stats, steps=5, poison=None):
    """`steps` train_iter calls on Small -> (parameters, [(preds, labels)] as train_iter returned them, the StepStats)."""
    from focus_amd import ops, train
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.utils import meters
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.NUM_CLASSES", 174, "MIXUP.ENABLE", bool(mix), "SOLVER.CLIP_GRAD_L2NORM", 0.0])
    torch.manual_seed(0)
    np.random.seed(0)
    m = Small().cuda()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    mixup_fn = train.build_mixup(cfg)
    loss_fun = ops.soft_target_ce if mix else (lambda p, l: ops.label_smoothing_ce(p, l, 0.1))
    stats = meters.StepStats("cuda") if use_stats else None
    g = torch.Generator().manual_seed(1)
    out = []
    for s in range(steps):
        x = torch.randn(8, 3, 2, 8, 8, generator=g)
        if poison == s:
            x[3, 0, 0, 0, 0] = float("nan")
        labels = torch.randperm(174, generator=g)[:8]                        # distinct: every mixed pair has two classes
        p, l, _ = train.train_iter(m, opt, loss_fun, [x.cuda()], labels.cuda(), {}, cfg, mixup_fn=mixup_fn, stats=stats)
        out.append((p.detach(), l))
    return [q.detach().clone() for q in m.parameters()], out, stats


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mixup"])
def test_train_iter_with_stats_is_the_same_training_and_the_same_numbers(mix):
    from focus_amd import train
    from focus_amd.slowfast.utils import metrics
    p0, out0, _ = _loop(mix, False)
    p1, out1, stats = _loop(mix, True)
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    correct = np.zeros(2)
    for (cp, cl), (rp, rl) in zip(out0, out1):
        if mix:
            assert rl.dim() == 2 and rl.dtype == torch.float32               # uncollapsed: what the step used
            top3 = rl.sort(dim=1, descending=True).values[:, :3]
            assert bool(((top3[:, 0] > top3[:, 1]) & (top3[:, 1] > top3[:, 2])).all())          # torch defines the order here
            assert bool(((cp == cp.gather(1, cl.view(-1, 1))).sum(1) == 1).all())
            tp, tl = train.mixup_collapse(rp, rl)
            assert torch.equal(tp, cp) and torch.equal(tl, cl)
        else:
            assert torch.equal(rp, cp) and torch.equal(rl, cl)
        correct += [float(x) for x in metrics.topks_correct(cp, cl, (1, 5))]
    w = stats.read()
    assert w["steps"] == 5 and w["samples"] == 40 and np.isfinite(w["loss"])
    assert w["top1_err"] == 100.0 * (40 - correct[0]) / 40 and w["top5_err"] == 100.0 * (40 - correct[1]) / 40
    e = stats.epoch_stats()
    assert e["top1_err"] == w["top1_err"] and e["samples"] == 40 and abs(e["loss"] - w["loss"]) < 1e-12      # equal batches


def test_a_nan_surfaces_at_the_next_read():
    with pytest.raises(RuntimeError, match="ERROR: Got NaN losses"):
        _loop(False, False, steps=3, poison=1)                                # the default path raises in the step
    _, out, stats = _loop(False, True, steps=3, poison=1)
    assert len(out) == 3                                                      # the loop went on
    with pytest.raises(RuntimeError, match=r"ERROR: Got NaN losses \(step 1\)"):
        stats.read()
    assert stats.read()["steps"] == 0                                         # the window was reset


def test_slot_train_step_stats_take_the_three_losses():
    """heads == 0: two iterations of slot_train_step on the small STEVE of tests/test_gpu_steve.py leave loss, mse and
    cross_entropy in the tables, bit-equal to the host's double sums of the returned scalars."""
    from test_gpu_steve import _steve_small
    from focus_amd.slowfast.models.optimizer import construct_optimizer_slot
    from focus_amd.slowfast.utils import meters
    from focus_amd.train import slot_train_step
    cfg, m = _steve_small(False)
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    cfg.SOLVER.CLIP_GRAD_L2NORM = 1.0
    m = m.to("cuda:0").train()
    opt = construct_optimizer_slot(m, cfg)
    video = torch.rand(2, 2, 3, 16, 16, generator=torch.Generator().manual_seed(0)).to("cuda:0")
    st = meters.StepStats("cuda:0", ks=(), aux_names=("mse", "cross_entropy"))
    sums = np.zeros(3)
    for step in range(2):
        loss, mse, ce, *_ = slot_train_step(m, opt, video, step, cfg, stats=st)
        for i, v in enumerate((loss, mse, ce)):
            sums[i] = sums[i] + np.float64(np.float32(float(v)))
    assert st.read() == {"loss": sums[0] / 2, "mse": sums[1] / 2, "cross_entropy": sums[2] / 2, "samples": 4, "steps": 2}
    st.update(None, None, torch.tensor(0.5, device="cuda"), (torch.tensor(0.25, device="cuda"), torch.tensor(1.0, device="cuda")), batch=3)
    assert st.read() == {"loss": 0.5, "mse": 0.25, "cross_entropy": 1.0, "samples": 3, "steps": 1}


class Scores(torch.nn.Module):
    def __init__(self, ek=False):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.ek = ek

    def forward(self, inputs, meta):
        f = inputs[0].flatten(1) + self.w
        if self.ek:
            return f[:, :9], {"verb": f[:, :9], "noun": f[:, 9:20]}
        return f[:, :9]


def test_eval_epoch_counts_every_batch_and_reads_once():
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.utils import metrics
    from focus_amd.train import eval_epoch
    g = torch.Generator().manual_seed(7)
    clips, lv, ln = torch.rand(10, 20, generator=g), torch.randint(0, 9, (10,), generator=g), torch.randint(0, 11, (10,), generator=g)
    cfg = get_cfg()
    loader = [([clips[i:i + 4]], lv[i:i + 4], None, {}) for i in range(0, 10, 4)]
    m = Scores().cuda().train()
    e = eval_epoch(loader, m, cfg)
    c1, c5 = (float(x) for x in metrics.topks_correct(clips[:, :9], lv, (1, 5)))
    assert not m.training and e["samples"] == 10 and e["steps"] == 3
    assert e["top1_err"] == 100.0 * (10 - c1) / 10 and e["top5_err"] == 100.0 * (10 - c5) / 10
    cfg.TRAIN.DATASET = "epickitchens"
    loader = [([clips[i:i + 4]], {"verb": lv[i:i + 4], "noun": ln[i:i + 4]}, None, {}) for i in range(0, 10, 4)]
    e = eval_epoch(loader, Scores(ek=True).cuda(), cfg)
    for name, acc in (("verb", metrics.topk_accuracies(clips[:, :9], lv, (1, 5))), ("noun", metrics.topk_accuracies(clips[:, 9:], ln, (1, 5))),
                      ("action", metrics.multitask_topk_accuracies((clips[:, :9], clips[:, 9:]), (lv, ln), (1, 5)))):
        for k, a in zip((1, 5), acc):
            assert abs(e["%s_top%d_acc" % (name, k)] - float(a)) < 1e-4, (name, k)


def test_perform_test_takes_the_ek_branch_and_the_device_meter():
    from focus_amd.slowfast.utils import meters
    from focus_amd.train import perform_test
    V, NC = 4, 3
    g = torch.Generator().manual_seed(5)
    clips = torch.rand(V * NC, 20, generator=g)
    lv, ln = torch.arange(V * NC) // NC % 9 + 1, torch.arange(V * NC) // NC % 11 + 1
    names = ["n%d" % i for i in range(V * NC)]
    loader = [([clips[i:i + 5]], {"verb": lv[i:i + 5], "noun": ln[i:i + 5]}, torch.arange(i, min(i + 5, V * NC)),
               {"narration_id": names[i:i + 5]}) for i in range(0, V * NC, 5)]
    meter = meters.EPICTestMeter(V, NC, (9, 11), len(loader), "cuda")
    st = perform_test(loader, Scores(ek=True).cuda(), meter, None)
    assert st is meter.stats and set(st) == {"split"} | {"%s_top%d_acc" % (n, k) for n in ("verb", "noun", "action") for k in (1, 5)}
    assert torch.allclose(meter.verb_video_preds.cpu(), clips[:, :9].view(V, NC, 9).sum(1), atol=1e-6)
    assert torch.allclose(meter.noun_video_preds.cpu(), clips[:, 9:].view(V, NC, 11).sum(1), atol=1e-6)
    assert list(meter.metadata) == [names[v * NC + NC - 1] for v in range(V)]
    loader = [([clips[i:i + 4]], lv[i:i + 4], torch.arange(i, min(i + 4, V * NC)), {}) for i in range(0, V * NC, 4)]
    dev, host = meters.DeviceTestMeter(V, NC, 9, len(loader), "cuda"), meters.TestMeter(V, NC, 9, len(loader))
    assert perform_test(loader, Scores().cuda(), dev, None) == perform_test(loader, Scores().cuda(), host, None)
    assert dev.video_preds.is_cuda and torch.allclose(dev.video_preds.cpu(), host.video_preds, atol=1e-6)


def test_operators_refuse_what_the_kernels_do_not_take(ops):
    acc_i = torch.zeros(16, dtype=torch.int64, device="cuda")
    acc_f = torch.zeros(8, dtype=torch.float64, device="cuda")
    x, l = torch.rand(4, 10, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for bad in (lambda: ops.topk_stats(acc_i, acc_f, x.half(), l), lambda: ops.topk_stats(acc_i, acc_f, x, l.int()),
                lambda: ops.topk_stats(acc_i, acc_f, x, l[:3]), lambda: ops.topk_stats(acc_i, acc_f, x, l, ks=(5, 1)),
                lambda: ops.topk_stats(acc_i, acc_f, x, l, ks=(1, 11)), lambda: ops.topk_stats(acc_i, acc_f, x.t(), l),
                lambda: ops.topk_stats(acc_i, acc_f, (x, x, x), (l, l, l)), lambda: ops.topk_stats(acc_i, acc_f, (x, x), (l, x)),
                lambda: ops.topk_stats(acc_i, acc_f, x, torch.rand(4, 9, device="cuda")), lambda: ops.topk_stats(acc_i[:8], acc_f, x, l),
                lambda: ops.topk_stats(acc_i, acc_f, x, l, losses=[torch.zeros(2, device="cuda")]),
                lambda: ops.topk_stats(acc_i, acc_f, losses=[torch.zeros((), device="cuda")])):
        with pytest.raises(ValueError, match="focus_amd: topk_stats"):
            bad()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_stats(acc_i, acc_f, x.cpu(), l.cpu())
    assert not acc_i.any() and not acc_f.any()
    d = dev_tables(2, 10)
    for bad in (lambda: ops.view_accumulate(x, l, l, 2, *d, mode="mean"), lambda: ops.view_accumulate(x.half(), l, l, 2, *d),
                lambda: ops.view_accumulate(x, l.int(), l, 2, *d), lambda: ops.view_accumulate(x, l, l[:3], 2, *d),
                lambda: ops.view_accumulate(x, l, l, 0, *d), lambda: ops.view_accumulate(x[:, :9], l, l, 2, *d),
                lambda: ops.view_accumulate(x, l, l, 2, d[0], d[1][:1], d[2], d[3])):
        with pytest.raises(ValueError, match="focus_amd: view_accumulate"):
            bad()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_accumulate(x.cpu(), l, l, 2, *d)
    assert not d[0].any() and int(d[3]) == 0
