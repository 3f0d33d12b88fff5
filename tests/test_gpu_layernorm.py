"""The seven kernels of csrc/layernorm.hip by the C ABI against tests/ln_ref.py in fp64, every route.

Inputs are rounded to the storage type first; every buffer a kernel writes is pre-filled with a quiet NaN no kernel
produces, with margins in front and behind, and every bit outside the output is pinned.  The bounds are derived in
ln_ref.py from operation counts (u = 2^-24) and every element is held to its own; the table, its routes, the reference and
the bounds are checked without a GPU in test_ln_ref_cpu.py.  Forward and backward are separate: the backward is given the
reference's mean and rstd rounded to fp32.

  forward / backward over ln_ref.CASES (one test per group of cases: a route and a D), the edge-row probes among them
  row blocks: T launches into one [B, T, rpb, D] buffer, each leaving the other frames alone, against the dense call
  row isolation: one Inf row changes no other row, once per LPR
  refused calls write nothing; no rows: the backward zero-fills
  through ops: layer_norm_frame, layer_norm_fork, deferred affine gradients, layer_norm_into, Prepared, an empty tensor

With -s every test prints the largest error / bound of each quantity it checks; the figures measured on an MI355X are the
comment at the end of this file."""
import ctypes

import pytest
import torch

import ln_ref as lr
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
OK, ERR_SHAPE, ERR_ALIGN, ERR_NULL = 0, -1, -3, -5
NAN_BITS = {F32: 0x7FC00123, BF16: 0x7FC1}       # the pre-fill of every output buffer: a quiet NaN no kernel produces
FRONT, TAIL = 8, 64                              # elements in front of the data and behind it (FRONT keeps 16 bytes)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _nan_buffer(n, dtype, d):
    return torch.full((n,), NAN_BITS[dtype], device=d, dtype=torch.int16 if dtype == BF16 else torch.int32).view(dtype)


def _is_prefill(t):
    return _bits(t) == NAN_BITS[t.dtype]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from focus_amd import _lib as L
    return L


def _dt(dtype):
    return _lib().BF16 if dtype == BF16 else _lib().F32


def _report(what, ratios):
    print("%-52s %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s: error / bound %s" % (what, bad)


class Dense:
    """n elements behind FRONT and in front of TAIL, all pre-filled; vals (optional) fill the n."""

    def __init__(self, n, dtype, d, vals=None):
        self.n, self.buf = n, _nan_buffer(FRONT + n + TAIL, dtype, d)
        if vals is not None:
            self.data().copy_(vals.reshape(-1))

    def data(self):
        return self.buf[FRONT:FRONT + self.n]

    def ptr(self):
        return self.buf.data_ptr() + FRONT * self.buf.element_size()

    def check_window(self, what, n=None):
        """The first n (default: all) elements are written, every bit around them is the pre-fill."""
        n = self.n if n is None else n
        assert not bool(_is_prefill(self.buf[FRONT:FRONT + n]).any()), what + ": not every element was written"
        assert bool(_is_prefill(self.buf[:FRONT]).all()) and bool(_is_prefill(self.buf[FRONT + n:]).all()), what + ": written outside"


class Rows:
    """The x (or dx) of a case: dense, or rows // rpb blocks of rpb rows xbs elements apart with the pointer at one frame,
    inside a pre-filled buffer; c['off'] moves the whole layout off its 16-byte alignment."""

    def __init__(self, c, d, vals=None):
        self.c, self.rows, self.D = c, c["rows"], c["D"]
        self.rpb, self.xbs = lr.rpb_of(c), lr.xbs_of(c)
        span = self.rows * self.D if c["rpb"] is None else (self.rows // self.rpb) * self.xbs
        self.base = FRONT + c["off"] + (0 if c["rpb"] is None else c["frame"] * self.rpb * self.D)
        self.buf = _nan_buffer(FRONT + c["off"] + span + TAIL, lr.torch_dtype(c), d)
        if vals is not None:
            self.put(vals)

    def ptr(self):
        return self.buf.data_ptr() + self.base * self.buf.element_size()

    def put(self, vals):
        if self.c["rpb"] is None:
            self.buf[self.base:self.base + self.rows * self.D].copy_(vals.reshape(-1))
        else:
            lr.scatter_rows(self.buf, self.base, vals, self.rpb, self.xbs)

    def get(self):
        if self.c["rpb"] is None:
            return self.buf[self.base:self.base + self.rows * self.D].view(self.rows, self.D)
        return lr.gather_rows(self.buf, self.base, self.rows, self.rpb, self.xbs, self.D)

    def check_window(self, what):
        """Exactly the rows are written: no pre-fill inside them, nothing but pre-fill outside."""
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        if self.c["rpb"] is None:
            inside[self.base:self.base + self.rows * self.D] = True
        else:
            lr.scatter_rows(inside, self.base, torch.ones(self.rows, self.D, dtype=torch.bool, device=self.buf.device), self.rpb, self.xbs)
        assert int(inside.sum()) == self.rows * self.D
        pre = _is_prefill(self.buf)
        assert not bool((pre & inside).any()), what + ": not every row was written"
        assert bool((pre | inside).all()), what + ": written outside the rows"


def _fwd_call(c, xptr, gamma, beta, y, mean, rstd, eps):
    lib, dt = _lib().lib(), _dt(lr.torch_dtype(c))
    if c["rpb"] is None:
        rc = lib.focus_layernorm_fwd(xptr, gamma.data_ptr(), beta.data_ptr(), y.ptr(), mean.ptr(), rstd.ptr(), c["rows"], c["D"],
                                     eps, dt, _stream())
    else:
        rc = lib.focus_layernorm_fwd_blocks(xptr, c["rpb"], lr.xbs_of(c), gamma.data_ptr(), beta.data_ptr(), y.ptr(), mean.ptr(),
                                            rstd.ptr(), c["rows"], c["D"], eps, dt, _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc


def _fwd_outputs(c, d):
    return (Dense(c["rows"] * c["D"], lr.torch_dtype(c), d), Dense(c["rows"], F32, d), Dense(c["rows"], F32, d))


def _bwd_call(c, dy, xptr, gamma, mean, rstd, dres, dxptr, dg, db, partial):
    lib, dt = _lib().lib(), _dt(lr.torch_dtype(c))
    dgp, dbp = (None, None) if dg is None else (dg.ptr(), db.ptr())
    if c["rpb"] is None:
        rc = lib.focus_layernorm_bwd(dy.data_ptr(), xptr, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                     None if dres is None else dres.data_ptr(), dxptr, dgp, dbp, partial.ptr(), c["rows"], c["D"],
                                     dt, _stream())
    else:
        assert dres is None
        rc = lib.focus_layernorm_bwd_blocks_strided(dy.data_ptr(), xptr, c["rpb"], lr.xbs_of(c), gamma.data_ptr(), mean.data_ptr(),
                                                    rstd.data_ptr(), dxptr, dgp, dbp, partial.ptr(), c["rows"], c["D"], dt, _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc


FWD_GROUPS = [g for g in lr.GROUPS if lr.group(g)[0]["dir"] == "fwd"]
BWD_GROUPS = [g for g in lr.GROUPS if any(c["dir"] == "bwd" for c in lr.group(g))]


@pytest.mark.parametrize("name", FWD_GROUPS)
def test_forward_values_window_repeat(name):
    d = dev()
    worst = {}
    for c in lr.group(name):
        what = lr.case_id(c)
        t = lr.inputs(c, d)
        X = Rows(c, d, t["x"])
        x0 = X.buf.clone()
        y, mean, rstd = _fwd_outputs(c, d)
        _fwd_call(c, X.ptr(), t["gamma"], t["beta"], y, mean, rstd, t["eps"])
        assert torch.equal(_bits(X.buf), _bits(x0)), what + ": the input was written"
        for o, n in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
            o.check_window("%s %s" % (what, n))
        y2, mean2, rstd2 = _fwd_outputs(c, d)
        _fwd_call(c, X.ptr(), t["gamma"], t["beta"], y2, mean2, rstd2, t["eps"])
        for a, b in ((y, y2), (mean, mean2), (rstd, rstd2)):
            assert torch.equal(_bits(a.buf), _bits(b.buf)), what + ": two launches differ"
        ratios = lr.fwd_ratios(c, t, dict(y=y.data().view(c["rows"], c["D"]), mean=mean.data(), rstd=rstd.data()))
        _report(what, ratios)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("# %-40s %s" % (name, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name", BWD_GROUPS)
def test_backward_values_window_partials(name):
    d = dev()
    worst = {}
    for c in lr.group(name):
        if c["dir"] != "bwd":
            continue
        what = lr.case_id(c)
        rows, D, dt = c["rows"], c["D"], lr.torch_dtype(c)
        t = lr.inputs(c, d)
        mean, rstd = lr.ref_stats(t, rows)
        nblk = _lib().lib().focus_layernorm_bwd_blocks(rows)
        assert nblk == lr.bwd_blocks(rows)
        X = Rows(c, d, t["x"])
        x0 = X.buf.clone()
        DX = Rows(c, d)
        dg, db, partial = Dense(D, F32, d), Dense(D, F32, d), Dense(2 * nblk * D, F32, d)
        _bwd_call(c, t["dy"], X.ptr(), t["gamma"], mean, rstd, t["dres"], DX.ptr(), dg, db, partial)
        assert torch.equal(_bits(X.buf), _bits(x0)), what + ": the input was written"
        DX.check_window(what + " dx")
        dg.check_window(what + " dgamma")
        db.check_window(what + " dbeta")
        partial.check_window(what + " partial")                     # all 2 * nblk * D entries, whether or not a block has rows
        # the protocol of the recurrent applications: no dgamma, no dbeta, the same partials and the same dx
        DX2, partial2 = Rows(c, d), Dense(2 * nblk * D, F32, d)
        _bwd_call(c, t["dy"], X.ptr(), t["gamma"], mean, rstd, t["dres"], DX2.ptr(), None, None, partial2)
        assert torch.equal(_bits(DX.buf), _bits(DX2.buf)), what + ": dx differs without dgamma / dbeta"
        assert torch.equal(_bits(partial.buf), _bits(partial2.buf)), what + ": partial differs without dgamma / dbeta"
        ratios = lr.bwd_ratios(c, t, mean, rstd, dict(dx=DX.get(), dgamma=dg.data(), dbeta=db.data(),
                                                      partial=partial.data().view(2, nblk, D)))
        _report(what, ratios)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("# %-40s %s" % (name, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


BLOCK_GROUPS = [g for g in lr.GROUPS if g.startswith("blocks-bwd-")]


@pytest.mark.parametrize("name", BLOCK_GROUPS)
def test_row_blocks_share_one_video_buffer(name):
    """x and dx as one [B, T, rpb, D] buffer each: the launches of the T frames (in the order 2, 0, 1) write their own rows
    only, all rows in the end, and each equals the dense call on a contiguous copy of the frame bit for bit -- forward and
    backward.  Blocks that are adjacent (T = 1) likewise."""
    d = dev()
    cases = [c for c in lr.group(name) if c["T"] == 3]
    c0 = cases[0]
    B, rpb, D, rows, dt = c0["rows"] // c0["rpb"], c0["rpb"], c0["D"], c0["rows"], lr.torch_dtype(c0)
    for T, frames in ((3, (2, 0, 1)), (1, (0,))):
        n = B * T * rpb * D
        xs = {f: lr.inputs(dict(c0, T=T, frame=f), d) for f in frames}
        video = Dense(n, dt, d)
        dxv = Dense(n, dt, d)
        view = lambda buf: buf.data().view(B, T, rpb, D)
        for f in frames:
            view(video)[:, f] = xs[f]["x"].view(B, rpb, D)
        v0 = video.buf.clone()
        for f in frames:
            c = dict(c0, T=T, frame=f)
            what = lr.case_id(c)
            t = xs[f]
            dense = dict(c, rpb=None, T=1, frame=0)
            assert lr.route_of(c) == lr.route_of(dense)
            fptr = lambda o: o.ptr() + f * rpb * D * o.buf.element_size()
            # forward
            y, mean, rstd = _fwd_outputs(c, d)
            _fwd_call(c, fptr(video), t["gamma"], t["beta"], y, mean, rstd, t["eps"])
            xc = view(video)[:, f].contiguous()
            assert torch.equal(_bits(xc.view(rows, D)), _bits(t["x"]))
            yd, meand, rstdd = _fwd_outputs(dense, d)
            _fwd_call(dense, xc.data_ptr(), t["gamma"], t["beta"], yd, meand, rstdd, t["eps"])
            for a, b2, n_ in ((y, yd, "y"), (mean, meand, "mean"), (rstd, rstdd, "rstd")):
                a.check_window("%s %s" % (what, n_))
                assert torch.equal(_bits(a.buf), _bits(b2.buf)), "%s: %s differs from the dense call" % (what, n_)
            # backward
            m, r = lr.ref_stats(t, rows)
            nblk = lr.bwd_blocks(rows)
            before = dxv.buf.clone()
            dg, db, partial = Dense(D, F32, d), Dense(D, F32, d), Dense(2 * nblk * D, F32, d)
            _bwd_call(c, t["dy"], fptr(video), t["gamma"], m, r, None, fptr(dxv), dg, db, partial)
            mine = torch.zeros(B, T, rpb, D, dtype=torch.bool, device=d)
            mine[:, f] = True
            mine = torch.cat([mine.new_zeros(FRONT), mine.view(-1), mine.new_zeros(TAIL)])
            assert torch.equal(_bits(dxv.buf)[~mine], _bits(before)[~mine]), what + ": another frame or a margin was written"
            assert not bool(_is_prefill(dxv.buf)[mine].any()), what + ": not every row of the frame was written"
            dxd = Dense(rows * D, dt, d)
            dgd, dbd, partiald = Dense(D, F32, d), Dense(D, F32, d), Dense(2 * nblk * D, F32, d)
            _bwd_call(dense, t["dy"], xc.data_ptr(), t["gamma"], m, r, None, dxd.ptr(), dgd, dbd, partiald)
            assert torch.equal(_bits(view(dxv)[:, f].reshape(-1)), _bits(dxd.data())), what + ": dx differs from the dense call"
            for a, b2, n_ in ((dg, dgd, "dgamma"), (db, dbd, "dbeta"), (partial, partiald, "partial")):
                assert torch.equal(_bits(a.buf), _bits(b2.buf)), "%s: %s differs from the dense call" % (what, n_)
            _report(what, lr.bwd_ratios(c, t, m, r, dict(dx=view(dxv)[:, f].reshape(rows, D), dgamma=dg.data(), dbeta=db.data())))
        assert torch.equal(_bits(video.buf), _bits(v0)), "the video was written"
        dxv.check_window("%s T %d dx of all frames" % (name, T))


ISOLATION = [("fp32", 9, 12, 4), ("bf16", 9, 260, 4), ("bf16", 4097, 64, 2051), ("bf16", 4097, 128, 2051),
             ("bf16", 4097, 256, 2051), ("bf16", 4097, 512, 2051), ("bf16", 4097, 1024, 2051)]


@pytest.mark.parametrize("dtype,rows,D,bad", ISOLATION, ids=lambda v: str(v))
def test_one_inf_row_changes_no_other_row(dtype, rows, D, bad):
    """Wave per row, and every LPR of the sub-wave kernels with the poisoned row in the middle of a wave's rows."""
    d = dev()
    res = []
    for poison in (False, True):
        cf = lr._case("fwd", dtype, rows, D, "isolation")
        t = lr.inputs(cf, d)
        if poison:
            t["x"][bad] = float("inf")
        X = Rows(cf, d, t["x"])
        y, mean, rstd = _fwd_outputs(cf, d)
        _fwd_call(cf, X.ptr(), t["gamma"], t["beta"], y, mean, rstd, t["eps"])
        cb = lr._case("bwd", dtype, rows, D, "isolation")
        tb = lr.inputs(cb, d)
        m, r = lr.ref_stats(tb, rows)                      # (the statistics of the rows without the poison)
        if poison:
            tb["x"][bad] = float("inf")
        XB, DX = Rows(cb, d, tb["x"]), Rows(cb, d)
        nblk = lr.bwd_blocks(rows)
        _bwd_call(cb, tb["dy"], XB.ptr(), tb["gamma"], m, r, None, DX.ptr(), None, None, Dense(2 * nblk * D, F32, d))
        res.append((y.data().view(rows, D).clone(), mean.data().clone(), rstd.data().clone(), DX.get().clone()))
    keep = torch.ones(rows, dtype=torch.bool, device=d)
    keep[bad] = False
    assert bool(torch.isnan(res[1][0][bad].float()).all()), "the y of the Inf row is not NaN"
    for a, b, n in zip(res[0], res[1], ("y", "mean", "rstd", "dx")):
        assert torch.equal(_bits(a[keep].contiguous()), _bits(b[keep].contiguous())), n + ": another row changed"


def test_refused_calls_write_nothing_and_no_rows_zero_fill():
    d = dev()
    lib, L = _lib().lib(), _lib()
    rows, D = 5, 8
    x = torch.ones(rows * D + 8, device=d)
    gamma = torch.ones(D, device=d)
    st = _stream()
    outs = lambda: [Dense(rows * D, F32, d), Dense(rows, F32, d), Dense(rows, F32, d), Dense(D, F32, d), Dense(D, F32, d), Dense(2 * 2 * D, F32, d)]
    p, g = x.data_ptr(), gamma.data_ptr()
    calls = [
        ("fwd D 6", lambda y, m, r, dg, db, pa: lib.focus_layernorm_fwd(p, g, g, y.ptr(), m.ptr(), r.ptr(), rows, 6, 1e-6, L.F32, st), ERR_SHAPE),
        ("fwd x 8 bytes", lambda y, m, r, dg, db, pa: lib.focus_layernorm_fwd(p + 8, g, g, y.ptr(), m.ptr(), r.ptr(), rows, D, 1e-6, L.F32, st), ERR_ALIGN),
        ("fwd blocks rpb 0", lambda y, m, r, dg, db, pa: lib.focus_layernorm_fwd_blocks(p, 0, 0, g, g, y.ptr(), m.ptr(), r.ptr(), rows, D, 1e-6, L.F32, st), ERR_SHAPE),
        ("bwd D 4100", lambda y, m, r, dg, db, pa: lib.focus_layernorm_bwd(p, p, g, p, p, None, y.ptr(), dg.ptr(), db.ptr(), pa.ptr(), rows, 4100, L.F32, st), ERR_SHAPE),
        ("bwd dy 8 bytes", lambda y, m, r, dg, db, pa: lib.focus_layernorm_bwd(p + 8, p, g, p, p, None, y.ptr(), dg.ptr(), db.ptr(), pa.ptr(), rows, D, L.F32, st), ERR_ALIGN),
        ("bwd dres 4 bytes", lambda y, m, r, dg, db, pa: lib.focus_layernorm_bwd(p, p, g, p, p, p + 4, y.ptr(), dg.ptr(), db.ptr(), pa.ptr(), rows, D, L.BF16, st), ERR_ALIGN),
        ("bwd dgamma alone", lambda y, m, r, dg, db, pa: lib.focus_layernorm_bwd(p, p, g, p, p, None, y.ptr(), dg.ptr(), None, pa.ptr(), rows, D, L.F32, st), ERR_NULL),
        ("bwd blocks xbs 6", lambda y, m, r, dg, db, pa: lib.focus_layernorm_bwd_blocks_strided(p, p, rows, 6, g, p, p, y.ptr(), dg.ptr(), db.ptr(), pa.ptr(), rows, D, L.F32, st), ERR_SHAPE),
        ("fwd rows 0", lambda y, m, r, dg, db, pa: lib.focus_layernorm_fwd(p, g, g, y.ptr(), m.ptr(), r.ptr(), 0, D, 1e-6, L.F32, st), OK),
    ]
    for what, call, want in calls:
        o = outs()
        rc = call(*o)
        torch.cuda.synchronize()
        assert rc == want, "%s: status %d, expected %d" % (what, rc, want)
        for b in o:
            assert bool(_is_prefill(b.buf).all()), what + ": an output was written"
    # no rows, backward: dgamma, dbeta and partial[2][1][D] are zero, nothing else is touched
    for finish in (True, False):
        y, m, r, dg, db, pa = outs()
        rc = lib.focus_layernorm_bwd(p, p, g, p, p, None, y.ptr(), dg.ptr() if finish else None, db.ptr() if finish else None,
                                     pa.ptr(), 0, D, L.F32, st)
        torch.cuda.synchronize()
        assert rc == OK
        assert bool(_is_prefill(y.buf).all())
        pa.check_window("partial of no rows", 2 * D)
        assert bool((_bits(pa.data()[:2 * D]) == 0).all())
        for b in (dg, db):
            if finish:
                b.check_window("no rows")
                assert bool((_bits(b.data()) == 0).all())
            else:
                assert bool(_is_prefill(b.buf).all())


# ---- through ops ----------------------------------------------------------------------------------------------------
def _ops_case(rows, D, dres=False):
    return lr._case("bwd", "bf16", rows, D, "ops", dres=dres, eps=1e-5)


def _bwd_ratios_from_saved(c, t, saved, got):
    """The backward against fp64 from the mean and rstd the forward kernel stored (saved_tensors[2:])."""
    return lr.bwd_ratios(c, t, saved[2], saved[3], got)


@pytest.mark.parametrize("N,skip", [(1025, None), (2051, None), (2051, 1)], ids=["2050 rows", "4102 rows", "4102 rows, frame 1 unused"])
def test_ops_layer_norm_frame(N, skip):
    """[2, 3, N, 192] bf16, the frames normalised in the order 2, 0, 1 through one FrameGrad: every y and the video's gradient
    rows against fp64, gamma / beta gradients as the sum over the frames; a frame that was never normalised has zero rows."""
    from focus_amd import ops
    d = dev()
    B, T, D = 2, 3, 192
    rows = B * N
    frames = [f for f in (2, 0, 1) if f != skip]
    cs = {f: dict(_ops_case(rows, D), rpb=N, T=T, frame=f) for f in frames}
    ts = {f: lr.inputs(cs[f], d) for f in frames}
    gamma, beta = (ts[frames[0]][k].clone().requires_grad_() for k in ("gamma", "beta"))
    video = torch.randn(B, T, N, D, device=d).bfloat16()
    for f in frames:
        video[:, f] = ts[f]["x"].view(B, N, D)
        ts[f]["gamma"], ts[f]["beta"] = gamma.detach(), beta.detach()
    video.requires_grad_()
    sh = ops.FrameGrad()
    ys = [ops.layer_norm_frame(video, f, gamma, beta, 1e-5, sh) for f in frames]
    saved = {f: y.grad_fn.saved_tensors for f, y in zip(frames, ys)}
    torch.autograd.backward(ys, [ts[f]["dy"].view(B, N, D) for f in frames])
    torch.cuda.synchronize()
    sg = sb = bg = bb = 0.0
    for f, y in zip(frames, ys):
        t = ts[f]
        fc = dict(cs[f], dir="fwd")
        _report("frame %d forward" % f, lr.fwd_ratios(fc, t, dict(y=y.detach().view(rows, D), mean=saved[f][2], rstd=saved[f][3])))
        _report("frame %d dx" % f, _bwd_ratios_from_saved(cs[f], t, saved[f], dict(dx=video.grad[:, f].reshape(rows, D))))
        _, dg, db = lr.bwd(t["dy"], t["x"], gamma.detach(), saved[f][2], saved[f][3])
        ag, ab = lr.col_scale(t["dy"], t["x"], saved[f][2], saved[f][3])
        k = (rows + lr.bwd_blocks(rows) + 16) * lr.U
        sg, sb, bg, bb = sg + dg, sb + db, bg + k * ag + len(frames) * lr.U * (dg.abs() + k * ag), bb + k * ab + len(frames) * lr.U * (db.abs() + k * ab)
    # the frames' fp32 gradients are added by autograd: T - 1 more roundings of at most the sum of their magnitudes
    _report("gamma, beta over the frames", dict(dgamma=lr.worst_ratio(gamma.grad, sg, bg), dbeta=lr.worst_ratio(beta.grad, sb, bb)))
    if skip is not None:
        assert bool((_bits(video.grad[:, skip].contiguous()) == 0).all()), "the rows of the unused frame are not zero"
    # inside deferred_wgrads: the same sums
    g2, b2 = (p.detach().clone().requires_grad_() for p in (gamma, beta))
    v2 = video.detach().clone().requires_grad_()
    with ops.deferred_wgrads():
        sh = ops.FrameGrad()
        ys2 = [ops.layer_norm_frame(v2, f, g2, b2, 1e-5, sh) for f in frames]
        torch.autograd.backward(ys2, [ts[f]["dy"].view(B, N, D) for f in frames])
    torch.cuda.synchronize()
    assert torch.equal(_bits(v2.grad), _bits(video.grad))
    _report("gamma, beta over the frames, deferred", dict(dgamma=lr.worst_ratio(g2.grad, sg, bg), dbeta=lr.worst_ratio(b2.grad, sb, bb)))


@pytest.mark.parametrize("rows,D", [(4107, 192), (131077, 64)])
def test_ops_layer_norm_fork_adds_dres(rows, D):
    from focus_amd import ops
    d = dev()
    c = _ops_case(rows, D, dres=True)
    t = lr.inputs(c, d)
    x = t["x"].clone().requires_grad_()
    gamma, beta = t["gamma"].clone().requires_grad_(), t["beta"].clone().requires_grad_()
    xres, h = ops.layer_norm_fork(x, gamma, beta, 1e-5)
    saved = h.grad_fn.saved_tensors
    torch.autograd.backward([xres, h], [t["dres"], t["dy"]])
    torch.cuda.synchronize()
    assert torch.equal(_bits(xres.detach()), _bits(t["x"]))
    _report("fork forward", lr.fwd_ratios(dict(c, dir="fwd"), t, dict(y=h.detach(), mean=saved[2], rstd=saved[3])))
    _report("fork backward", _bwd_ratios_from_saved(c, t, saved, dict(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)))


def test_ops_forward_only_entries_and_an_empty_tensor():
    """layer_norm_into and Prepared.layer_norm are ops.layer_norm's forward bit for bit and fill their statistics; an empty
    tensor runs forward and backward, with zero parameter gradients."""
    from focus_amd import ops
    d = dev()
    for rows, D in ((352, 192), (4100, 192)):
        c = lr._case("fwd", "bf16", rows, D, "ops", eps=1e-5)
        t = lr.inputs(c, d)
        x = t["x"].clone().requires_grad_()
        y = ops.layer_norm(x, t["gamma"], t["beta"], 1e-5)
        saved = y.grad_fn.saved_tensors
        out, stats = Dense(rows * D, BF16, d), Dense(2 * rows, F32, d)
        ops.layer_norm_into(t["x"], t["gamma"], t["beta"], 1e-5, out.data().view(rows, D), stats.data().view(2, rows))
        pre = ops.Prepared()
        out2 = Dense(rows * D, BF16, d)
        pre.layer_norm(t["x"], t["gamma"], t["beta"], 1e-5, out2.data().view(rows, D))
        pre.run()
        torch.cuda.synchronize()
        for o in (out, out2):
            o.check_window("layer_norm_into / Prepared")
            assert torch.equal(_bits(o.data()), _bits(y.detach().reshape(-1)))
        stats.check_window("stats")
        assert torch.equal(_bits(stats.data()[:rows]), _bits(saved[2])) and torch.equal(_bits(stats.data()[rows:]), _bits(saved[3]))
        pstats = pre.keep[-1][4]
        assert torch.equal(_bits(pstats[0]), _bits(saved[2])) and torch.equal(_bits(pstats[1]), _bits(saved[3]))
        _report("ops.layer_norm %dx%d" % (rows, D), lr.fwd_ratios(c, t, dict(y=y.detach(), mean=saved[2], rstd=saved[3])))
    for dtype in (F32, BF16):
        D = 16
        x = torch.empty(0, D, device=d, dtype=dtype, requires_grad=True)
        gamma, beta = torch.ones(D, device=d, requires_grad=True), torch.zeros(D, device=d, requires_grad=True)
        y = ops.layer_norm(x, gamma, beta, 1e-6)
        assert y.shape == (0, D)
        y.float().sum().backward()
        torch.cuda.synchronize()
        assert x.grad.shape == (0, D)
        assert bool((gamma.grad == 0).all()) and bool((beta.grad == 0).all())


# Measured on an MI355X: the largest error / bound of every checked quantity, per group of cases (a group: one route and one D,
# or what its name says; the lines starting with "# " of a run with -s), then the lines the tests through ops print.  finish
# dgamma / dbeta: dgamma, dbeta against the fp64 column sums of `partial`.  y and dx in bf16 sit at 0.99: half an ulp of the
# type is the bound, and some element of a few thousand always comes close to a tie; the fp32 arithmetic under it uses the
# fraction of its bound the fp32 rows show.  dgamma / dbeta over >= 2049 rows of random dy use under 0.001 of (rows + nblk + 16) u
# sum |terms| -- a worst case for any order of summation, of which roundings of random sign use little -- which is why the
# edge-row probes exist: there a dropped or doubled row is a fifth of the sum.
#   blocks-fwd-bf16-2x2051x192               mean 0.004  rstd 0.024  y 0.995
#   blocks-fwd-bf16-3x1025x196               mean 0.003  rstd 0.021  y 0.996
#   blocks-fwd-bf16-3x2051x520               mean 0.002  rstd 0.009  y 0.995
#   blocks-fwd-bf16-3x7x260                  mean 0.001  rstd 0.014  y 0.987
#   blocks-fwd-fp32-3x1025x196               mean 0.007  rstd 0.020  y 0.793
#   blocks-fwd-fp32-3x7x12                   mean 0.073  rstd 0.114  y 0.623
#   cond-fwd-bf16                            mean 0.000  rstd 0.017  y 0.980
#   cond-fwd-fp32                            mean 0.003  rstd 0.011  y 0.221
#   sub-fwd-D1024                            mean 0.001  rstd 0.031  y 0.996
#   sub-fwd-D128                             mean 0.004  rstd 0.136  y 0.996
#   sub-fwd-D136                             mean 0.004  rstd 0.125  y 0.996
#   sub-fwd-D256                             mean 0.002  rstd 0.091  y 0.996
#   sub-fwd-D264                             mean 0.003  rstd 0.088  y 0.996
#   sub-fwd-D512                             mean 0.001  rstd 0.055  y 0.996
#   sub-fwd-D520                             mean 0.001  rstd 0.053  y 0.996
#   sub-fwd-D64                              mean 0.010  rstd 0.178  y 0.996
#   sub-fwd-D72                              mean 0.010  rstd 0.179  y 0.996
#   sub-fwd-D8                               mean 0.071  rstd 0.304  y 0.996
#   trip2-fwd-D136                           mean 0.006  rstd 0.035  y 0.996
#   trip2-fwd-D264                           mean 0.003  rstd 0.020  y 0.996
#   trip2-fwd-D520                           mean 0.002  rstd 0.010  y 0.995
#   trip2-fwd-D72                            mean 0.016  rstd 0.064  y 0.996
#   trip2-fwd-D8                             mean 0.097  rstd 0.337  y 0.996
#   wave-fwd-bf16-4100                       mean 0.004  rstd 0.022  y 0.995
#   wave-fwd-bf16-D1024                      mean 0.000  rstd 0.021  y 0.990
#   wave-fwd-bf16-D1028                      mean 0.001  rstd 0.020  y 0.981
#   wave-fwd-bf16-D12                        mean 0.034  rstd 0.088  y 0.928
#   wave-fwd-bf16-D2048                      mean 0.000  rstd 0.006  y 0.980
#   wave-fwd-bf16-D2052                      mean 0.000  rstd 0.007  y 0.985
#   wave-fwd-bf16-D252                       mean 0.001  rstd 0.065  y 0.977
#   wave-fwd-bf16-D256                       mean 0.001  rstd 0.059  y 0.983
#   wave-fwd-bf16-D260                       mean 0.002  rstd 0.022  y 0.980
#   wave-fwd-bf16-D4                         mean 0.000  rstd 0.162  y 0.716
#   wave-fwd-bf16-D4096                      mean 0.000  rstd 0.004  y 0.978
#   wave-fwd-bf16-D768                       mean 0.000  rstd 0.025  y 0.974
#   wave-fwd-bf16-D772                       mean 0.000  rstd 0.019  y 0.989
#   wave-fwd-fp32-D1024                      mean 0.001  rstd 0.018  y 0.862
#   wave-fwd-fp32-D1028                      mean 0.001  rstd 0.023  y 0.399
#   wave-fwd-fp32-D12                        mean 0.044  rstd 0.114  y 0.582
#   wave-fwd-fp32-D2048                      mean 0.001  rstd 0.007  y 0.475
#   wave-fwd-fp32-D2052                      mean 0.000  rstd 0.003  y 0.435
#   wave-fwd-fp32-D252                       mean 0.003  rstd 0.050  y 0.455
#   wave-fwd-fp32-D256                       mean 0.003  rstd 0.064  y 0.419
#   wave-fwd-fp32-D260                       mean 0.003  rstd 0.040  y 0.460
#   wave-fwd-fp32-D4                         mean 0.196  rstd 0.172  y 0.443
#   wave-fwd-fp32-D4096                      mean 0.000  rstd 0.005  y 0.416
#   wave-fwd-fp32-D768                       mean 0.001  rstd 0.016  y 0.529
#   wave-fwd-fp32-D772                       mean 0.001  rstd 0.028  y 0.279
#   blocks-bwd-bf16-2x2051x192               dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.002  sum partial[0] 0.000  sum partial[1] 0.000
#   blocks-bwd-bf16-3x1025x196               dbeta 0.000  dgamma 0.000  dx 0.994  finish dbeta 0.000  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   blocks-bwd-bf16-3x2051x520               dbeta 0.000  dgamma 0.000  dx 0.994  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   blocks-bwd-bf16-3x7x260                  dbeta 0.000  dgamma 0.046  dx 0.990  finish dbeta 0.000  finish dgamma 0.078  sum partial[0] 0.028  sum partial[1] 0.000
#   blocks-bwd-fp32-3x1025x196               dbeta 0.000  dgamma 0.000  dx 0.112  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   blocks-bwd-fp32-3x7x12                   dbeta 0.017  dgamma 0.019  dx 0.150  finish dbeta 0.052  finish dgamma 0.061  sum partial[0] 0.014  sum partial[1] 0.012
#   edge                                     dbeta 0.020  dgamma 0.035  dx 0.960  finish dbeta 0.029  finish dgamma 0.027  sum partial[0] 0.043  sum partial[1] 0.000
#   sub-bwd-D1024                            dbeta 0.000  dgamma 0.000  dx 0.994  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D128                             dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.002  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D136                             dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.002  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D256                             dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.002  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D264                             dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D512                             dbeta 0.000  dgamma 0.000  dx 0.994  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D520                             dbeta 0.000  dgamma 0.000  dx 0.994  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D64                              dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.003  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D72                              dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.003  sum partial[0] 0.000  sum partial[1] 0.000
#   sub-bwd-D8                               dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wave-bwd-bf16-2049                       dbeta 0.000  dgamma 0.000  dx 0.992  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wave-bwd-bf16-4100                       dbeta 0.000  dgamma 0.000  dx 0.994  finish dbeta 0.000  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wave-bwd-bf16-D1024                      dbeta 0.000  dgamma 0.125  dx 0.979  finish dbeta 0.000  finish dgamma 0.078  sum partial[0] 0.125  sum partial[1] 0.000
#   wave-bwd-bf16-D1028                      dbeta 0.000  dgamma 0.133  dx 0.978  finish dbeta 0.000  finish dgamma 0.092  sum partial[0] 0.133  sum partial[1] 0.000
#   wave-bwd-bf16-D12                        dbeta 0.000  dgamma 0.078  dx 0.955  finish dbeta 0.000  finish dgamma 0.043  sum partial[0] 0.078  sum partial[1] 0.000
#   wave-bwd-bf16-D2048                      dbeta 0.011  dgamma 0.150  dx 0.975  finish dbeta 0.000  finish dgamma 0.085  sum partial[0] 0.150  sum partial[1] 0.011
#   wave-bwd-bf16-D2052                      dbeta 0.000  dgamma 0.142  dx 0.981  finish dbeta 0.000  finish dgamma 0.090  sum partial[0] 0.142  sum partial[1] 0.000
#   wave-bwd-bf16-D252                       dbeta 0.000  dgamma 0.153  dx 0.968  finish dbeta 0.000  finish dgamma 0.080  sum partial[0] 0.153  sum partial[1] 0.000
#   wave-bwd-bf16-D256                       dbeta 0.000  dgamma 0.120  dx 0.977  finish dbeta 0.000  finish dgamma 0.087  sum partial[0] 0.120  sum partial[1] 0.000
#   wave-bwd-bf16-D260                       dbeta 0.000  dgamma 0.153  dx 0.979  finish dbeta 0.000  finish dgamma 0.075  sum partial[0] 0.153  sum partial[1] 0.000
#   wave-bwd-bf16-D4                         dbeta 0.000  dgamma 0.038  dx 0.928  finish dbeta 0.000  finish dgamma 0.060  sum partial[0] 0.038  sum partial[1] 0.000
#   wave-bwd-bf16-D4096                      dbeta 0.000  dgamma 0.134  dx 0.976  finish dbeta 0.000  finish dgamma 0.095  sum partial[0] 0.134  sum partial[1] 0.000
#   wave-bwd-bf16-D768                       dbeta 0.006  dgamma 0.115  dx 0.975  finish dbeta 0.000  finish dgamma 0.091  sum partial[0] 0.115  sum partial[1] 0.006
#   wave-bwd-bf16-D772                       dbeta 0.000  dgamma 0.125  dx 0.991  finish dbeta 0.000  finish dgamma 0.094  sum partial[0] 0.125  sum partial[1] 0.000
#   wave-bwd-fp32-2049                       dbeta 0.000  dgamma 0.000  dx 0.329  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wave-bwd-fp32-4100                       dbeta 0.000  dgamma 0.000  dx 0.380  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wave-bwd-fp32-D1024                      dbeta 0.093  dgamma 0.116  dx 0.014  finish dbeta 0.079  finish dgamma 0.086  sum partial[0] 0.116  sum partial[1] 0.091
#   wave-bwd-fp32-D1028                      dbeta 0.086  dgamma 0.133  dx 0.016  finish dbeta 0.094  finish dgamma 0.100  sum partial[0] 0.133  sum partial[1] 0.081
#   wave-bwd-fp32-D12                        dbeta 0.112  dgamma 0.112  dx 0.172  finish dbeta 0.051  finish dgamma 0.050  sum partial[0] 0.112  sum partial[1] 0.112
#   wave-bwd-fp32-D2048                      dbeta 0.081  dgamma 0.148  dx 0.010  finish dbeta 0.087  finish dgamma 0.088  sum partial[0] 0.148  sum partial[1] 0.081
#   wave-bwd-fp32-D2052                      dbeta 0.099  dgamma 0.143  dx 0.011  finish dbeta 0.080  finish dgamma 0.092  sum partial[0] 0.143  sum partial[1] 0.099
#   wave-bwd-fp32-D252                       dbeta 0.087  dgamma 0.115  dx 0.053  finish dbeta 0.079  finish dgamma 0.065  sum partial[0] 0.115  sum partial[1] 0.087
#   wave-bwd-fp32-D256                       dbeta 0.076  dgamma 0.110  dx 0.039  finish dbeta 0.080  finish dgamma 0.084  sum partial[0] 0.110  sum partial[1] 0.067
#   wave-bwd-fp32-D260                       dbeta 0.080  dgamma 0.139  dx 0.041  finish dbeta 0.079  finish dgamma 0.086  sum partial[0] 0.139  sum partial[1] 0.080
#   wave-bwd-fp32-D4                         dbeta 0.068  dgamma 0.062  dx 0.162  finish dbeta 0.041  finish dgamma 0.055  sum partial[0] 0.062  sum partial[1] 0.068
#   wave-bwd-fp32-D4096                      dbeta 0.105  dgamma 0.149  dx 0.005  finish dbeta 0.097  finish dgamma 0.090  sum partial[0] 0.149  sum partial[1] 0.105
#   wave-bwd-fp32-D768                       dbeta 0.080  dgamma 0.118  dx 0.023  finish dbeta 0.077  finish dgamma 0.080  sum partial[0] 0.118  sum partial[1] 0.075
#   wave-bwd-fp32-D772                       dbeta 0.082  dgamma 0.115  dx 0.016  finish dbeta 0.089  finish dgamma 0.088  sum partial[0] 0.115  sum partial[1] 0.082
#   wide-bwd-D1024                           dbeta 0.000  dgamma 0.000  dx 0.994  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wide-bwd-D128                            dbeta 0.000  dgamma 0.000  dx 0.996  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wide-bwd-D256                            dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wide-bwd-D512                            dbeta 0.000  dgamma 0.000  dx 0.995  finish dbeta 0.001  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
#   wide-bwd-D64                             dbeta 0.000  dgamma 0.000  dx 0.996  finish dbeta 0.000  finish dgamma 0.001  sum partial[0] 0.000  sum partial[1] 0.000
# through ops (test_ops_layer_norm_frame: 2050 rows, 4102 rows, 4102 rows without frame 1; _fork: 4107 x 192, 131077 x 64):
#   frame 2 forward                                      mean 0.004  rstd 0.020  y 0.995
#   frame 2 dx                                           dx 0.993
#   frame 0 forward                                      mean 0.003  rstd 0.021  y 0.996
#   frame 0 dx                                           dx 0.994
#   frame 1 forward                                      mean 0.003  rstd 0.020  y 0.995
#   frame 1 dx                                           dx 0.994
#   gamma, beta over the frames                          dbeta 0.000  dgamma 0.000
#   gamma, beta over the frames, deferred                dbeta 0.000  dgamma 0.000
#   frame 2 forward                                      mean 0.005  rstd 0.023  y 0.994
#   frame 2 dx                                           dx 0.994
#   frame 0 forward                                      mean 0.004  rstd 0.021  y 0.995
#   frame 0 dx                                           dx 0.993
#   frame 1 forward                                      mean 0.003  rstd 0.022  y 0.996
#   frame 1 dx                                           dx 0.994
#   gamma, beta over the frames                          dbeta 0.000  dgamma 0.000
#   gamma, beta over the frames, deferred                dbeta 0.000  dgamma 0.000
#   frame 2 forward                                      mean 0.005  rstd 0.023  y 0.994
#   frame 2 dx                                           dx 0.994
#   frame 0 forward                                      mean 0.004  rstd 0.021  y 0.995
#   frame 0 dx                                           dx 0.993
#   gamma, beta over the frames                          dbeta 0.000  dgamma 0.000
#   gamma, beta over the frames, deferred                dbeta 0.000  dgamma 0.000
#   fork forward                                         mean 0.004  rstd 0.026  y 0.995
#   fork backward                                        dbeta 0.000  dgamma 0.000  dx 0.995
#   fork forward                                         mean 0.010  rstd 0.060  y 0.996
#   fork backward                                        dbeta 0.000  dgamma 0.000  dx 0.996
#   ops.layer_norm 352x192                               mean 0.004  rstd 0.020  y 0.992
#   ops.layer_norm 4100x192                              mean 0.005  rstd 0.022  y 0.994
