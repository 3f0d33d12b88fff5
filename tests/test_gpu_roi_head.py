"""csrc/roi_head.hip by the C ABI against tests/roi_head_ref.py in fp64, then ops.roi_head_pool, ResNetRoIHead inside a small
detection MViT, one training step and the test loop.

Inputs are rounded to the storage type first.  Outputs are pre-filled with a quiet NaN no kernel produces; the token buffer of
the backward has guard rows in front and behind and (cls = 1) a cls row per sample, all of which keep their pre-fill.  The
bounds are derived in roi_head_ref.py and every element is held to its own; the table, the twin and the bounds are checked
without a GPU in test_roi_head_ref_cpu.py.  With -s every test prints error / bound of what it checks."""
import ctypes

import numpy as np
import pytest
import torch

import roi_head_ref as R
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
OK, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_NULL, ERR_WORKSPACE = 0, -1, -2, -3, -5, -6
NAN_BITS = {F32: 0x7FC00123, BF16: 0x7FC1}
GUARD = 2                                                    # guard rows of C elements in front of and behind the tokens


def _L():
    from focus_amd import _lib
    return _lib


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
    return _L().BF16 if dtype == BF16 else _L().F32


def _nan(n, dtype):
    return torch.full((n,), NAN_BITS[dtype], device=dev(), dtype=torch.int16 if dtype == BF16 else torch.int32).view(dtype)


def _prefill(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32) == NAN_BITS[t.dtype]


def _report(what, ratios):
    print("%-58s %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s: error / bound %s" % (what, bad)


class Stream:
    """A token buffer [GUARD rows | B x (cls + N) rows | GUARD rows] of C elements, pre-filled; tokens(): the [B, cls + N, C] view."""

    def __init__(self, B, N, C, cls, dtype, x=None):
        self.B, self.N, self.C, self.cls = B, N, C, cls
        self.buf = _nan((2 * GUARD + B * (cls + N)) * C, dtype)
        if x is not None:
            self.tokens()[:, cls:].copy_(x)

    def tokens(self):
        return self.buf[GUARD * self.C:-GUARD * self.C].view(self.B, self.cls + self.N, self.C)

    def ptr(self):
        return _p(self.buf, (GUARD + self.cls) * self.C)

    def stride(self):
        return (self.cls + self.N) * self.C

    def untouched_outside(self):
        ok = bool(_prefill(self.buf[:GUARD * self.C]).all()) and bool(_prefill(self.buf[-GUARD * self.C:]).all())
        return ok and (self.cls == 0 or bool(_prefill(self.tokens()[:, :self.cls]).all()))


def _fwd_call(c, x, rois, st=None):
    """-> status, pooled, arg, the stream."""
    a, dt = R.args_of(c), R.torch_dtype(c)
    N = a["T"] * a["H"] * a["W"]
    st = st or Stream(R.B, N, c["C"], c["cls"], dt, x.to(dev()))
    K = rois.shape[0]
    r = torch.from_numpy(rois).to(dev())
    pooled = _nan(max(K, 1) * c["C"], dt).view(max(K, 1), c["C"])[:K]
    arg = torch.full((max(K, 1), c["C"]), -7, device=dev(), dtype=torch.int32)[:K]
    L = _L().lib()
    nb = L.focus_roi_head_workspace_bytes(R.B, a["H"], a["W"], c["C"])
    ws = torch.empty(nb // 4, device=dev(), dtype=F32)
    s = L.focus_roi_head_fwd(st.ptr(), st.stride(), _p(r), _p(pooled), _p(arg), _p(ws), nb, R.B, a["T"], a["H"], a["W"], c["C"], K,
                             a["PH"], a["PW"], a["scale"], a["sampling_ratio"], int(a["aligned"]), _dt(dt), _stream())
    return s, pooled, arg, st


def _bwd_call(c, dp, arg, rois):
    a, dt = R.args_of(c), R.torch_dtype(c)
    st = Stream(R.B, a["T"] * a["H"] * a["W"], c["C"], c["cls"], dt)
    K = rois.shape[0]
    r = torch.from_numpy(rois).to(dev()) if K else None
    s = _L().lib().focus_roi_head_bwd(_p(dp) if K else None, _p(arg) if K else None, _p(r), st.ptr(), st.stride(), R.B, a["T"], a["H"],
                                      a["W"], c["C"], K, a["PH"], a["PW"], a["scale"], a["sampling_ratio"], int(a["aligned"]),
                                      _dt(dt), _stream())
    return s, st


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_kernels_against_the_twin(c):
    x, dp, rois = R.inputs(c)
    a = R.args_of(c)
    bf = c["dtype"] == "bf16"
    geo = (a["T"], a["H"], a["W"], a["PH"], a["PW"], a["scale"], a["sampling_ratio"], a["aligned"])
    pooled, bins, _ = R.fwd(x, rois, **a)
    s, got, arg, st = _fwd_call(c, x, rois)
    assert s == OK
    fb = R.fwd_bound(x, rois, *geo, False)
    ratios = dict(pooled=R.worst_ratio(got, pooled, R.fwd_bound(x, rois, *geo, bf, pooled)), arg=R.arg_ratio(arg, bins, fb))
    assert bool((arg[4] == 0).all()) and bool((got[4] == 0).all())                      # the box outside the frame
    # the integer side: the twin's fp32 geometry (which produced `bins`) is focus_roi_align_indices'
    from focus_amd import ops
    g_dev, n_dev = ops.roi_align_indices(torch.from_numpy(rois[:, 1:].copy()).to(dev()), a["H"], a["W"], a["PH"], a["PW"], a["scale"],
                                         a["sampling_ratio"], a["aligned"])
    g_ref, n_ref = R.indices(rois, a["scale"], a["PH"], a["PW"], a["sampling_ratio"], a["aligned"], a["H"], a["W"])
    assert (g_dev.cpu().numpy() == g_ref).all() and (n_dev.cpu().numpy() == n_ref).all()
    # backward, fed the kernel's own arg
    dpd = dp.to(dev())
    s, sb = _bwd_call(c, dpd, arg, rois)
    assert s == OK
    dx = sb.tokens()[:, c["cls"]:]
    bgeo = (R.B,) + geo
    want = R.bwd(dp, arg, rois, *bgeo)
    ratios["dx"] = R.worst_ratio(dx, want, R.bwd_bound(dp, arg, rois, *bgeo, bf, want))
    assert bool((dx[1] == 0).all()), "image 1 has no box: zeros"
    assert sb.untouched_outside() and st.untouched_outside()
    s, sb2 = _bwd_call(c, dpd, arg, rois)
    assert s == OK and torch.equal(sb2.tokens()[:, c["cls"]:].contiguous().view(torch.uint8),
                                   dx.contiguous().view(torch.uint8)), "two runs are bit-equal"
    _report(R.case_id(c), ratios)


def _case(**kw):
    c = dict(dtype="fp32", T=2, H=5, W=9, C=8, PH=3, PW=2, cls=1, aligned=1, sr=0)
    c.update(kw)
    return c


def test_no_boxes():
    c = _case()
    x, _, rois = R.inputs(c)
    s, pooled, arg, st = _fwd_call(c, x, rois[:0])
    assert s == OK and pooled.numel() == 0 and st.untouched_outside()
    s, sb = _bwd_call(c, None, None, rois[:0])
    assert s == OK and bool((sb.tokens()[:, 1:] == 0).all()) and sb.untouched_outside()
    from focus_amd import ops
    tok = torch.randn(R.B, 1 + 2 * 45, 8, device=dev(), requires_grad=True)
    y = ops.roi_head_pool(tok, torch.zeros(0, 5), 2, 5, 9, 3, 2, 1.0 / 16)
    assert y.shape == (0, 8)
    y.sum().backward()
    assert tok.grad.shape == tok.shape and bool((tok.grad == 0).all())


def test_refusals_write_nothing():
    c = _case()
    x, dp, rois = R.inputs(c)
    a, L = R.args_of(c), _L().lib()
    st = Stream(R.B, 2 * 45, 8, 1, F32, x.to(dev()))
    r = torch.from_numpy(rois).to(dev())
    pooled, arg = _nan(9 * 8, F32).view(9, 8), torch.full((9, 8), -7, device=dev(), dtype=torch.int32)
    nb = L.focus_roi_head_workspace_bytes(R.B, 5, 9, 8)
    ws = torch.empty(nb // 4 + 4, device=dev(), dtype=F32)
    base = dict(x=st.ptr(), bs=st.stride(), rois=_p(r), ws=_p(ws), nb=nb, B=R.B, T=2, H=5, W=9, C=8, K=9, PH=3, PW=2, dt=_L().F32)

    def fwd(**kw):
        v = dict(base, **kw)
        return L.focus_roi_head_fwd(v["x"], v["bs"], v["rois"], _p(pooled), _p(arg), v["ws"], v["nb"], v["B"], v["T"], v["H"], v["W"],
                                    v["C"], v["K"], v["PH"], v["PW"], a["scale"], 0, 1, v["dt"], _stream())

    def bwd(**kw):
        v = dict(base, **kw)
        return L.focus_roi_head_bwd(_p(pooled), _p(arg), v["rois"], v["x"], v["bs"], v["B"], v["T"], v["H"], v["W"], v["C"], v["K"],
                                    v["PH"], v["PW"], a["scale"], 0, 1, v["dt"], _stream())
    for f in (fwd, bwd):
        assert f(dt=_L().FP8_E4M3) == ERR_DTYPE and f(dt=7) == ERR_DTYPE
        assert f(C=6) == ERR_ALIGN                                                    # C % 4
        assert f(bs=st.stride() + 2) == ERR_ALIGN
        assert f(x=_p(st.buf, (GUARD + 1) * 8 + 1)) == ERR_ALIGN                      # one element off
        assert f(T=1025) == ERR_SHAPE and f(PH=33, PW=32) == ERR_SHAPE and f(H=23, W=23) == ERR_SHAPE
        assert f(K=65536) == ERR_SHAPE and f(K=-1) == ERR_SHAPE and f(T=0) == ERR_SHAPE and f(PH=0) == ERR_SHAPE
        assert f(bs=2 * 45 * 8 - 4) == ERR_SHAPE                                      # samples would overlap
        assert f(rois=None) == ERR_NULL
    assert fwd(ws=None) == ERR_NULL and fwd(nb=nb - 4) == ERR_WORKSPACE and fwd(ws=_p(ws, 1)) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(_prefill(pooled).all()) and bool((arg == -7).all())
    assert torch.equal(st.tokens()[:, 1:], x.to(dev())) and st.untouched_outside()


def test_ops_matches_the_c_abi_and_refuses_a_bad_batch_index():
    from focus_amd import ops
    for c in (_case(), _case(dtype="bf16", cls=0, T=8, H=14, W=14, C=40, PH=7, PW=7)):
        x, dp, rois = R.inputs(c)
        a = R.args_of(c)
        s, pooled, arg, st = _fwd_call(c, x, rois)
        assert s == OK
        tok = st.tokens().clone()
        if c["cls"]:
            tok[:, 0] = 1.0
        tok.requires_grad_(True)
        # boxes as a host tensor: checked on the host, copied by ops
        got, garg = ops.roi_head_pool(tok, torch.from_numpy(rois), a["T"], a["H"], a["W"], a["PH"], a["PW"], a["scale"],
                                      sampling_ratio=a["sampling_ratio"], aligned=a["aligned"], cls=c["cls"], return_arg=True)
        assert torch.equal(got, pooled) and torch.equal(garg, arg)
        got.backward(dp.to(dev()))
        s, sb = _bwd_call(c, dp.to(dev()), arg, rois)
        assert s == OK and torch.equal(tok.grad[:, c["cls"]:], sb.tokens()[:, c["cls"]:])
        if c["cls"]:
            assert bool((tok.grad[:, 0] == 0).all())
        for bad in (3.0, -1.0, 0.5, float("nan")):
            r = torch.from_numpy(rois.copy())
            r[2, 0] = bad
            with pytest.raises(ValueError, match="batch index"):
                ops.roi_head_pool(tok, r, a["T"], a["H"], a["W"], a["PH"], a["PW"], a["scale"], cls=c["cls"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.roi_head_pool(torch.zeros(1, 46, 8), torch.zeros(1, 5), 1, 5, 9, 3, 2, 1 / 16.0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_ops_against_the_composition_of_existing_ops(dtype):
    """mean over T in torch -> ops.roi_align_tokens -> ops.cell_amax on inputs whose top two bins are separated (so both paths
    route the gradient through the same bin).  Each path is within its own bound of fp64, so they are within the sum."""
    from focus_amd import ops
    T, H, W, C, PH, PW = 2, 7, 7, 8, 3, 2
    x, rois, Bn = R.separated_inputs(T, H, W, C, PH, PW, dtype=dtype)
    scale = 1.0 / R.SCALE_FACTOR
    geo = (T, H, W, PH, PW, scale, 0, True)
    pooled, bins, arg = R.fwd(x, rois, *geo)
    sep = R.separation(bins)
    bf = dtype == BF16
    fb = R.fwd_bound(x, rois, *geo, bf, pooled)
    X = float(x.abs().max())
    extra_f = 2 * R.BF * X if bf else 0.0                                               # the composition's rounded mean and cells
    # no path can take another bin: two bins' worth of the largest error of either path is below the lead
    assert sep > 0.4 and sep > 2 * (R.fwd_bound(x, rois, *geo, False).max() + extra_f)
    dp = torch.randn(rois.shape[0], C, generator=torch.Generator().manual_seed(5)).to(dtype)
    xa = x.to(dev()).requires_grad_(True)
    ya, arga = ops.roi_head_pool(xa, torch.from_numpy(rois), *geo[:6], sampling_ratio=0, aligned=True, cls=0, return_arg=True)
    ya.backward(dp.to(dev()))
    xb = x.to(dev()).requires_grad_(True)
    mean = xb.float().reshape(Bn, T, H * W, C).mean(1).to(dtype)                        # (bf16: one more rounding of the mean)
    r = torch.from_numpy(rois).to(dev())
    cells = ops.roi_align_tokens(mean, r[:, 1:].contiguous(), r[:, 0].to(torch.int32), H, W, PH, PW, scale, 0, True)
    yb = ops.cell_amax(cells)
    yb.backward(dp.to(dev()))
    assert (arga.cpu().numpy() == arg).all()
    want_dx = R.bwd(dp, arg, rois, Bn, *geo)
    bb = R.bwd_bound(dp, arg, rois, Bn, *geo, bf, want_dx)
    extra_b = 2 * R.BF * np.abs(want_dx) if bf else 0.0                                 # its rounded d(cells) and d(mean)
    ratios = dict(fused_fwd=R.worst_ratio(ya, pooled, fb), fused_bwd=R.worst_ratio(xa.grad, want_dx, bb),
                  composed_fwd=R.worst_ratio(yb, pooled, fb + extra_f), composed_bwd=R.worst_ratio(xb.grad, want_dx, bb + extra_b),
                  fused_vs_composed_fwd=R.worst_ratio(ya, yb.detach().double().cpu().numpy(), 2 * fb + extra_f),
                  fused_vs_composed_bwd=R.worst_ratio(xa.grad, xb.grad.double().cpu().numpy(), 2 * bb + extra_b))
    _report("fused vs mean -> roi_align_tokens -> cell_amax, %s" % dtype, ratios)


# ---- the model, the step, the test loop ---------------------------------------------------------------------------------
def _det_cfg(extra=()):
    from test_roi_head_ref_cpu import _det_cfg as base
    return base(["SOLVER.OPTIMIZING_METHOD", "sgd", "SOLVER.BASE_LR", 0.1, "SOLVER.WEIGHT_DECAY", 0.0] + list(extra))


def _det_batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, 4, 32, 32, generator=g)
    boxes = torch.tensor([[1, 2.0, 3.0, 30.0, 28.0], [0, 0.0, 0.0, 32.0, 32.0], [1, 10.0, 4.0, 18.0, 25.0]])
    labels = (torch.rand(3, 5, generator=g) > 0.6).float()
    return x, boxes, labels


def _model(extra=()):
    from focus_amd.slowfast.models import build_model
    torch.manual_seed(0)
    return build_model(_det_cfg(extra))


def test_detection_mvit_head_against_the_twin():
    """oracle.mvit_forward does not expose its features, so the head alone is compared, on the model's own normalised tokens:
    twin pooling in fp64 -> projection -> sigmoid."""
    m = _model().eval()
    x, boxes, _ = _det_batch()
    seen = {}
    hook = m.head.register_forward_hook(lambda _m, inp, out: seen.update(tokens=inp[0][0].detach(), out=out.detach()))
    with torch.no_grad():
        y = m([x.to(dev())], {}, bboxes=boxes)
    hook.remove()
    tok = seen["tokens"]
    assert tok.shape == (2, 1 + 2 * 8 * 8, 16) and y.shape == (3, 5) and torch.equal(y, seen["out"])
    rois = boxes.numpy()
    geo = (2, 8, 8, 3, 3, 0.25, 0, True)
    pooled, _, _ = R.fwd(tok[:, 1:], rois, *geo)
    fb = R.fwd_bound(tok[:, 1:], rois, *geo, False)
    w, b = m.head.projection.weight.detach().double().cpu().numpy(), m.head.projection.bias.detach().double().cpu().numpy()
    want = 1.0 / (1.0 + np.exp(-(pooled @ w.T + b)))
    # |d sigmoid| <= |d logit| / 4; the logit: the pooled bound through |w|, plus an fp32 dot product of 16 terms
    bound = 0.25 * (fb @ np.abs(w).T + (16 + 2) * R.U * (np.abs(pooled) @ np.abs(w).T + np.abs(b))) + 4 * R.U
    _report("detection MViT head: scores", dict(scores=R.worst_ratio(y, want, bound)))
    with torch.no_grad():
        assert torch.equal(m([x.to(dev())], {}, bboxes=boxes.to(dev())), y)            # boxes already on the device
    with pytest.raises(ValueError, match="bboxes"):
        m([x.to(dev())], {})


def test_detection_train_iter_sgd():
    from focus_amd.slowfast.models.losses import get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    from focus_amd.train import train_iter
    cfg = _det_cfg()
    m = _model().train()
    opt = construct_optimizer(m, cfg)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    x, boxes, labels = _det_batch()
    w0 = m.head.projection.weight.detach().clone()
    preds, _, loss = train_iter(m, opt, loss_fun, [x.to(dev())], labels.to(dev()), {"boxes": boxes.to(dev())}, cfg)
    assert preds.shape == (3, 5) and bool(((preds > 0) & (preds < 1)).all())           # the activation runs in training too
    assert np.isfinite(float(loss.detach()))
    missing = [n for n, p in m.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, "parameters without a gradient: %s" % missing
    assert float((m.head.projection.weight.detach() - w0).abs().max()) > 0


def test_detection_head_dropout():
    m = _model(["MODEL.DROPOUT_RATE", 0.5])
    assert m.head.dropout_rate == 0.5
    x, boxes, _ = _det_batch()
    with torch.no_grad():
        m.eval()
        e1, e2 = m([x.to(dev())], {}, bboxes=boxes), m([x.to(dev())], {}, bboxes=boxes)
        m.train()
        t1 = m([x.to(dev())], {}, bboxes=boxes)
    assert torch.equal(e1, e2) and not torch.equal(t1, e1)


def test_perform_test_hands_the_meter_host_tensors():
    from focus_amd.train import eval_epoch, perform_test

    class Meter:
        def __init__(self):
            self.seen, self.done = [], False

        def update_stats(self, preds, ori_boxes, metadata):
            self.seen.append((preds, ori_boxes, metadata))

        def finalize_metrics(self):
            self.done = True
            return "done"
    cfg = _det_cfg()
    m = _model()
    x, boxes, labels = _det_batch()
    meta = {"boxes": boxes, "ori_boxes": boxes * 2.0, "metadata": torch.tensor([[7, 1], [7, 2], [9, 1]])}
    loader = [([x], labels, torch.arange(2), meta), ([x.flip(0)], labels, torch.arange(2), meta)]
    meter = Meter()
    assert perform_test(loader, m, meter, cfg) == "done" and meter.done and len(meter.seen) == 2
    for preds, ori, md in meter.seen:
        assert preds.shape == (3, 5) and ori.shape == (3, 5) and md.shape == (3, 2)
        assert preds.device.type == ori.device.type == md.device.type == "cpu"
        assert torch.equal(ori, boxes * 2.0) and torch.equal(md, meta["metadata"])
    assert not torch.equal(meter.seen[0][0], meter.seen[1][0])
    val = Meter()
    assert eval_epoch(loader, m, cfg, stats=val) is val and len(val.seen) == 2
    assert torch.equal(val.seen[0][0], meter.seen[0][0])
    bad = dict(meta, boxes=torch.tensor([[2, 0.0, 0.0, 8.0, 8.0]]))
    with pytest.raises(ValueError, match="batch index"):
        perform_test([([x], labels, torch.arange(2), bad)], m, Meter(), cfg)
