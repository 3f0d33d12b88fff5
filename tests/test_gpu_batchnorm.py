"""The kernels of csrc/batchnorm.hip by the C ABI against tests/bn_ref.py in fp64, and the operators over them.

Inputs are rounded to the storage type first; every buffer a kernel writes is pre-filled with a quiet NaN no kernel
produces (int8: a code no window position has), with margins in front and behind, and every bit outside the output is pinned.
Each stage is compared with its fp64 formula on the kernel's OWN stored inputs (the apply on the stored mean and rstd, the
backward on the stored y as well), against bounds derived in bn_ref.py from operation counts; every element is held to its
own bound.  The references, the bounds and the mutants are checked without a GPU in test_bn_ref_cpu.py.

  statistics: rows 2, 63, 64, 65, the first R whose partials exceed one wave and (C = 256) the first R with a second
    grid-stride trip, both read from focus_bn_blocks; running buffers; two runs bit-identical; the cancellation case
  apply / backward: relu x residual x frozen in every combination; dres = g bit for bit; dgamma, dbeta bit-repeatable
  max-pool: values and indices exact, no ties in the random inputs (asserted), the tie rule on all-zero and post-ReLU maps
  operators: NCHW-strided and channels-last inputs give the same bits; values and gradients against fp64; autocast; eval mode

With -s every test prints the largest error / bound of each quantity it checks."""
import ctypes

import pytest
import torch

import bn_ref as br
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

F32, BF16, F64, I8 = torch.float32, torch.bfloat16, torch.float64, torch.int8
OK = 0
FRONT, TAIL = 16, 64
_INT = {F32: torch.int32, BF16: torch.int16, I8: torch.int8}
NAN_BITS = {F32: 0x7FC00123, BF16: 0x7FC1, I8: 0x5A}


def _lib():
    from focus_amd import _lib as L
    return L


def _dt(dtype):
    return _lib().BF16 if dtype == BF16 else _lib().F32


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(what, ratios):
    print("%-58s %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s: error / bound %s" % (what, bad)


def _ratio(got, ref, bound):
    """Largest error / bound over all elements; an element with a zero bound has to be exact."""
    err = (got.to(F64) - ref).abs()
    assert bool(torch.isfinite(got.to(F64)).all()), "not finite"
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, 2.0), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


class Buf:
    """n elements behind FRONT and in front of TAIL pre-filled elements; vals (optional) fill the n."""

    def __init__(self, n, dtype, d, vals=None):
        self.n, self.dtype = n, dtype
        self.buf = torch.full((FRONT + n + TAIL,), NAN_BITS[dtype], device=d, dtype=_INT[dtype]).view(dtype)
        if vals is not None:
            self.data().copy_(vals.reshape(-1))

    def data(self):
        return self.buf[FRONT:FRONT + self.n]

    def ptr(self):
        return self.buf.data_ptr() + FRONT * self.buf.element_size()

    def _pre(self, t):
        return t.view(_INT[self.dtype]) == NAN_BITS[self.dtype]

    def check(self, what, written=True):
        """Nothing outside the n elements is written; written: every one of the n is; written=False: none is."""
        assert bool(self._pre(self.buf[:FRONT]).all()) and bool(self._pre(self.buf[FRONT + self.n:]).all()), what + ": written outside"
        if written is True:
            assert not bool(self._pre(self.data()).any()), what + ": not every element was written"
        elif written is False:
            assert bool(self._pre(self.data()).all()), what + ": a switched-off output was written"


def _workspace(R, C, d):
    nbytes = _lib().lib().focus_bn_workspace_bytes(R, C)
    assert nbytes == br.workspace_bytes(R, C)
    return Buf(nbytes // 4, F32, d)


def _stats(x, R, C, dtype, d, running=None):
    """-> mean, rstd, (running_mean, running_var) Bufs after focus_bn_stats."""
    mean, rstd, ws = Buf(C, F32, d), Buf(C, F32, d), _workspace(R, C, d)
    rm = rv = None
    if running is not None:
        rm, rv = Buf(C, F32, d, running[0]), Buf(C, F32, d, running[1])
    rc = _lib().lib().focus_bn_stats(x.data_ptr(), mean.ptr(), rstd.ptr(), rm.ptr() if rm else None, rv.ptr() if rv else None,
                                     ws.ptr(), R, C, br.EPS, br.MOMENTUM, _dt(dtype), _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    mean.check("mean"), rstd.check("rstd"), ws.check("workspace", written=None)
    if rm:
        rm.check("running_mean"), rv.check("running_var")
    return mean, rstd, rm, rv


def _rows_list(C):
    blocks = _lib().lib().focus_bn_blocks
    rows = list(br.ROWS_SMALL) + [br.first_rows_with_blocks_over(64, blocks)]
    assert blocks(rows[-1]) > 64 and blocks(rows[-1] - 1) <= 64            # stage 2: more partials than one wave holds
    if C == 256:
        R = br.first_rows_with_second_trip(C, blocks)
        assert R > br.UNROLL * blocks(R) * br.rpb(C) and R - 1 <= br.UNROLL * blocks(R - 1) * br.rpb(C)
        rows.append(R)
    for R in rows:
        assert blocks(R) == br.blocks(R)
    return rows


@pytest.mark.parametrize("C", br.CHANNELS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_statistics_running_buffers_repeatability(dtype, C):
    d = dev()
    worst = {}
    for R in _rows_list(C):
        t = br.inputs(R, C, dtype, seed=2, device=d)
        x0 = t["x"].clone()
        mean, rstd, rm, rv = _stats(t["x"], R, C, dtype, d, (t["running_mean"], t["running_var"]))
        assert torch.equal(t["x"], x0)
        sb = br.stats_bounds(t["x"], br.EPS)
        rm_ref, rv_ref, bm, bv = br.running_bounds(t["running_mean"], t["running_var"], sb, R, br.MOMENTUM)
        r = dict(mean=_ratio(mean.data(), sb["ref_mean"], sb["mean"]), rstd=_ratio(rstd.data(), sb["ref_rstd"], sb["rstd"]),
                 run_mean=_ratio(rm.data(), rm_ref, bm), run_var=_ratio(rv.data(), rv_ref, bv))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # a second run gives the same bits; without running buffers the statistics are the same bits too
        mean2, rstd2, rm2, rv2 = _stats(t["x"], R, C, dtype, d, (t["running_mean"], t["running_var"]))
        mean3, rstd3, _, _ = _stats(t["x"], R, C, dtype, d, None)
        for a, b in ((mean, mean2), (rstd, rstd2), (rm, rm2), (rv, rv2), (mean, mean3), (rstd, rstd3)):
            assert torch.equal(a.data().view(torch.int32), b.data().view(torch.int32)), "R=%d: not bit-repeatable" % R
    _report("statistics C=%d %s rows %s" % (C, dtype, _rows_list(C)), worst)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_statistics_cancellation(dtype):
    """Per-channel mean 100, std 0.1: E[x^2] - E[x]^2 in fp32 is far outside these bounds (test_bn_ref_cpu.py)."""
    d = dev()
    worst = {}
    for R, C in ((4096, 64), (64, 256), (32768, 8)):
        t = br.inputs(R, C, dtype, seed=3, kind="offset", device=d)
        mean, rstd, _, _ = _stats(t["x"], R, C, dtype, d)
        sb = br.stats_bounds(t["x"], br.EPS)
        worst["mean %dx%d" % (R, C)] = _ratio(mean.data(), sb["ref_mean"], sb["mean"])
        worst["rstd %dx%d" % (R, C)] = _ratio(rstd.data(), sb["ref_rstd"], sb["rstd"])
    _report("cancellation %s" % dtype, worst)


def _apply(t, mean, rstd, R, C, dtype, d, relu, res):
    y = Buf(R * C, dtype, d)
    rc = _lib().lib().focus_bn_apply(t["x"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), t["gamma"].data_ptr(),
                                     t["beta"].data_ptr(), t["res"].data_ptr() if res else None, y.ptr(), R, C, int(relu),
                                     _dt(dtype), _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    y.check("y")
    return y


def _backward(t, ydata, mean, rstd, R, C, dtype, d, relu, res, frozen):
    dx, dres, dg, db, ws = Buf(R * C, dtype, d), Buf(R * C, dtype, d), Buf(C, F32, d), Buf(C, F32, d), _workspace(R, C, d)
    rc = _lib().lib().focus_bn_bwd(t["dy"].data_ptr(), t["x"].data_ptr(), ydata.data_ptr() if relu else None, mean.data_ptr(),
                                   rstd.data_ptr(), t["gamma"].data_ptr(), dx.ptr(), dres.ptr() if res else None, dg.ptr(),
                                   db.ptr(), ws.ptr(), R, C, int(relu), int(frozen), _dt(dtype), _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    dx.check("dx"), dg.check("dgamma"), db.check("dbeta"), ws.check("workspace", written=None)
    dres.check("dres", written=bool(res))                              # a switched-off output keeps its NaN guard
    return dx, dres, dg, db


@pytest.mark.parametrize("C", br.CHANNELS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_apply_and_backward_every_flag_combination(dtype, C):
    d = dev()
    worst = {}
    rows = _rows_list(C)
    for R in rows:
        big = R > 4096                                                  # the second-trip shape: one combination of each stage
        t = br.inputs(R, C, dtype, seed=4, device=d)
        keep = {k: v.clone() for k, v in t.items()}
        mean_b, rstd_b, _, _ = _stats(t["x"], R, C, dtype, d)
        batch = (mean_b.data().clone(), rstd_b.data().clone())
        frozen_stats = (t["running_mean"].clone(), torch.rsqrt(t["running_var"] + br.EPS))
        for relu, res, frozen in br.FLAGS:
            if big and not (relu and res and not frozen):
                continue
            mean, rstd = frozen_stats if frozen else batch
            y = _apply(t, mean, rstd, R, C, dtype, d, relu, res)
            yv = y.data().view(R, C)
            r_ = t["res"] if res else None
            ry = _ratio(yv, br.fwd(t["x"], mean, rstd, t["gamma"], t["beta"], r_, relu),
                        br.fwd_bound(t["x"], mean, rstd, t["gamma"], t["beta"], r_, relu, dtype == BF16))
            if relu:
                assert float(yv.float().min()) >= 0.0
            dx, dres, dg, db = _backward(t, yv, mean, rstd, R, C, dtype, d, relu, res, frozen)
            dx_ref, g_ref, dg_ref, db_ref = br.bwd(t["dy"], t["x"], yv, mean, rstd, t["gamma"], relu, frozen)
            bx, bg, bb = br.bwd_bounds(t["dy"], t["x"], yv, mean, rstd, t["gamma"], relu, frozen, dtype == BF16)
            r = dict(y=ry, dx=_ratio(dx.data().view(R, C), dx_ref, bx), dgamma=_ratio(dg.data(), dg_ref, bg),
                     dbeta=_ratio(db.data(), db_ref, bb))
            if res:
                assert torch.equal(dres.data().view(R, C).to(F64), g_ref), "dres is not g"
            dx2, dres2, dg2, db2 = _backward(t, yv, mean, rstd, R, C, dtype, d, relu, res, frozen)
            for a, b in ((dg, dg2), (db, db2), (dx, dx2)):
                assert torch.equal(a.data().view(_INT[a.dtype]), b.data().view(_INT[b.dtype])), "R=%d: not bit-repeatable" % R
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
        for k, v in t.items():
            assert torch.equal(v, keep[k]), "input %s was written" % k
    _report("apply / backward C=%d %s rows %s" % (C, dtype, rows), worst)


def _pool(x, N, H, W, C, dtype, d, dy=None):
    OH, OW = br.pool_out(H), br.pool_out(W)
    n_out = N * OH * OW * C
    y, idx = Buf(n_out, dtype, d), Buf(n_out, I8, d)
    lib = _lib().lib()
    rc = lib.focus_maxpool_fwd(x.data_ptr(), y.ptr(), idx.ptr(), N, H, W, C, _dt(dtype), _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    y.check("pool y"), idx.check("pool idx")
    dx = None
    if dy is not None:
        dx = Buf(N * H * W * C, dtype, d)
        rc = lib.focus_maxpool_bwd(dy.data_ptr(), idx.ptr(), dx.ptr(), N, H, W, C, _dt(dtype), _stream())
        torch.cuda.synchronize()
        assert rc == OK, rc
        dx.check("pool dx")
    return y.data().view(N, OH, OW, C), idx.data().view(N, OH, OW, C), dx


def _no_tie_map(N, H, W, C, dtype, g):
    """[N, H, W, C] random values without a tie in any 3x3 window.  fp32: normal draws.  bf16 holds 8 significant bits, and
    normal draws rounded to it do tie: there, integers p + 16 q / 8 with p a random permutation of 0..15 per (n, c) laid out
    over (h mod 4, w mod 4) -- distinct modulo 16 inside any 3x3 window -- and q a random integer in [-4, 3]: exact in bf16."""
    if dtype == F32:
        return torch.randn(N, H, W, C, generator=g)
    perm = torch.rand(N, 16, C, generator=g).argsort(dim=1)                              # [N, 16, C]
    cell = (torch.arange(H)[:, None] % 4) * 4 + torch.arange(W)[None, :] % 4           # [H, W]
    p = perm[:, cell.reshape(-1)].view(N, H, W, C)
    q = torch.randint(-4, 4, (N, H, W, C), generator=g)
    x = (p + 16 * q).float() / 8
    assert torch.equal(x.to(BF16).float(), x)
    return x.to(BF16)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_max_pool_values_indices_backward(dtype):
    d = dev()
    worst = 0.0
    g = torch.Generator().manual_seed(11)
    for (H, W) in br.POOL_HW:
        for N in br.POOL_N:
            for C in (8, 64):
                OH, OW = br.pool_out(H), br.pool_out(W)
                x = _no_tie_map(N, H, W, C, dtype, g).to(d)
                assert br.window_ties(x.to(F64)) == 0
                dy = torch.randn(N, OH, OW, C, generator=g).to(dtype).to(d)
                y, idx, dx = _pool(x, N, H, W, C, dtype, d, dy)
                y_ref, idx_ref = br.maxpool(x.to(F64))
                assert torch.equal(y.to(F64), y_ref) and torch.equal(idx, idx_ref), (N, H, W, C)
                dx_ref, sc = br.maxpool_bwd(dy, idx, H, W)
                worst = max(worst, _ratio(dx.data().view(N, H, W, C), dx_ref, br.pool_bwd_bound(dx_ref, sc, dtype == BF16)))
    _report("max-pool backward %s" % dtype, dict(dx=worst))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_max_pool_tie_rule(dtype):
    """The first maximum in row-major window order, padded positions skipped: read off the stored indices."""
    d = dev()
    g = torch.Generator().manual_seed(12)
    zero = torch.zeros(1, 4, 4, 8, dtype=dtype, device=d)
    y, idx, dx = _pool(zero, 1, 4, 4, 8, dtype, d, torch.ones(1, 2, 2, 8, dtype=dtype, device=d))
    assert torch.equal(idx, br.maxpool(zero.to(F64))[1]) and not bool(y.any())
    assert dx.data().view(4, 4, 8)[:, :, 0].nonzero().tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    for (H, W) in ((8, 8), (3, 5), (16, 16)):
        x = torch.randn(3, H, W, 64, generator=g).clamp_min(0).to(dtype).to(d)
        assert br.window_ties(x.to(F64)) > 0
        y, idx, _ = _pool(x, 3, H, W, 64, dtype, d)
        y_ref, idx_ref = br.maxpool(x.to(F64))
        assert torch.equal(y.to(F64), y_ref) and torch.equal(idx, idx_ref)
        assert not torch.equal(idx, br.maxpool(x.to(F64), last=True)[1])
    neg = (-torch.rand(2, 3, 5, 8, generator=g) - 1.0).to(dtype).to(d)            # a padded position must not win with a 0
    y, idx, _ = _pool(neg, 2, 3, 5, 8, dtype, d)
    assert torch.equal(y.to(F64), br.maxpool(neg.to(F64))[0]) and float(y.float().max()) < 0


# ---- the operators ---------------------------------------------------------------------------------------------------------
def _nrel(a, b):
    return float((a.to(F64) - b).norm() / b.norm().clamp_min(1e-300))


def _layouts(x):
    """The same values as an NCHW-contiguous tensor, a channels-last one and a strided NCHW view."""
    x = x.detach()
    wide = torch.zeros(x.shape[0], x.shape[1], x.shape[2], x.shape[3] + 3, dtype=x.dtype, device=x.device)
    wide[..., :x.shape[3]] = x
    return dict(nchw=x.clone(memory_format=torch.contiguous_format), channels_last=x.contiguous(memory_format=torch.channels_last), strided=wide[..., :x.shape[3]])


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_ops_batch_norm_against_fp64(dtype, training):
    """ops.batch_norm on three memory layouts: the same bits from each, and values, running buffers and all four gradients
    against the fp64 formulas (mask from the operator's own output).  Bound: the project's fp32 parity bound 1e-3 on the
    norm-wise relative error, plus the bf16 rounding of a stored activation (2^-8 relative) where the result is bf16."""
    from focus_amd import ops
    d = dev()
    N, C, H, W = 3, 64, 5, 7
    R = N * H * W
    t = br.inputs(R, C, dtype, seed=5, device=d)
    nchw = lambda rows: rows.view(N, H, W, C).permute(0, 3, 1, 2)
    rows = lambda t4: t4.permute(0, 2, 3, 1).reshape(R, C)
    tol = 1e-3 + (2.0 ** -8 if dtype == BF16 else 0.0)
    outs = {}
    for name in ("nchw", "channels_last", "strided"):
        x = _layouts(nchw(t["x"]))[name].requires_grad_()
        res = _layouts(nchw(t["res"]))[name].requires_grad_()
        ct = _layouts(nchw(t["dy"]))[name]
        gamma, beta = t["gamma"].clone().requires_grad_(), t["beta"].clone().requires_grad_()
        rm, rv = t["running_mean"].clone(), t["running_var"].clone()
        y = ops.batch_norm(x, gamma, beta, rm, rv, training, br.MOMENTUM, br.EPS, relu=True, residual=res)
        assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
        y.backward(ct)
        assert gamma.grad.dtype == F32 and x.grad.dtype == dtype and res.grad.dtype == dtype
        outs[name] = (y.detach(), x.grad, res.grad, gamma.grad, beta.grad, rm, rv)
    for name in ("channels_last", "strided"):
        for a, b in zip(outs["nchw"], outs[name]):
            assert torch.equal(a, b), name
    y, dx, dres, dg, db, rm, rv = outs["nchw"]
    if training:
        mean, var = br.stats(t["x"])
        rm_ref, rv_ref = br.running_update(t["running_mean"], t["running_var"], mean, var, R, br.MOMENTUM)
    else:
        mean, var = t["running_mean"].to(F64), t["running_var"].to(F64)
        rm_ref, rv_ref = mean, var
    rstd = 1.0 / torch.sqrt(var + br.EPS)
    y_ref = br.fwd(t["x"], mean, rstd, t["gamma"], t["beta"], t["res"], True)
    dx_ref, g_ref, dg_ref, db_ref = br.bwd(t["dy"], t["x"], rows(y), mean, rstd, t["gamma"], True, frozen=not training)
    r = dict(y=_nrel(rows(y), y_ref) / tol, dx=_nrel(rows(dx), dx_ref) / tol, dgamma=_nrel(dg, dg_ref) / 1e-3,
             dbeta=_nrel(db, db_ref) / 1e-3, run_mean=_nrel(rm, rm_ref) / 1e-3, run_var=_nrel(rv, rv_ref) / 1e-3)
    assert torch.equal(rows(dres).to(F64), g_ref)
    _report("ops.batch_norm %s %s" % (dtype, "train" if training else "eval"), r)


def test_ops_batch_norm_under_autocast_and_refusals():
    from focus_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(6)
    conv = torch.nn.Conv2d(3, 64, 3, 1, 1).to(d).to(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(64).to(d)
    x = torch.rand(2, 3, 8, 8, generator=g).to(d)
    with torch.autocast("cuda", dtype=BF16):
        h = conv(x)
        y = ops.batch_norm(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, bn.momentum, bn.eps, relu=True)
        z = ops.max_pool_3x3_s2(y)
    assert h.dtype == BF16 and y.dtype == BF16 and z.dtype == BF16 and tuple(z.shape) == (2, 64, 4, 4)
    z.float().square().sum().backward()
    assert bn.weight.grad.dtype == F32 and bn.running_mean.dtype == F32 and conv.weight.grad is not None
    assert bool(torch.isfinite(bn.weight.grad).all()) and float(bn.running_mean.abs().max()) > 0
    with pytest.raises(RuntimeError, match="momentum=None"):
        ops.batch_norm(h.detach(), bn.weight, bn.bias, bn.running_mean, bn.running_var, True, None, bn.eps)
    with pytest.raises(RuntimeError):
        ops.batch_norm(h.detach()[:, :60], bn.weight[:60], bn.bias[:60], None, None, True, 0.1, bn.eps)      # C % 8
    with pytest.raises(RuntimeError):
        ops.batch_norm(h.detach()[:1, :, :1, :1], bn.weight, bn.bias, None, None, True, 0.1, bn.eps)         # one row: as torch


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_ops_max_pool_against_fp64(dtype):
    from focus_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(7)
    N, C, H, W = 3, 64, 7, 10
    x0 = torch.randn(N, C, H, W, generator=g).clamp_min(0).to(dtype).to(d)                 # post-ReLU: ties
    ct = torch.randn(N, C, br.pool_out(H), br.pool_out(W), generator=g).to(dtype).to(d)
    outs = {}
    for name in ("nchw", "channels_last", "strided"):
        x = _layouts(x0)[name].requires_grad_()
        y = ops.max_pool_3x3_s2(x)
        assert y.is_contiguous(memory_format=torch.channels_last) and y.dtype == dtype
        y.backward(_layouts(ct)[name])
        outs[name] = (y.detach(), x.grad)
    for name in ("channels_last", "strided"):
        assert torch.equal(outs["nchw"][0], outs[name][0]) and torch.equal(outs["nchw"][1], outs[name][1])
    nhwc = lambda t4: t4.permute(0, 2, 3, 1)
    y_ref, idx = br.maxpool(nhwc(x0).to(F64))
    assert torch.equal(nhwc(outs["nchw"][0]).to(F64), y_ref)
    dx_ref, sc = br.maxpool_bwd(nhwc(ct), idx, H, W)
    _report("ops.max_pool_3x3_s2 %s" % dtype,
            dict(dx=_ratio(nhwc(outs["nchw"][1]), dx_ref, br.pool_bwd_bound(dx_ref, sc, dtype == BF16))))
    # ATen itself, same tie rule: the same pooled values and the same gradient up to the order of <= 4 additions
    xa = x0.clone().requires_grad_()
    ya = torch.nn.functional.max_pool2d(xa, 3, 2, 1)
    ya.backward(ct)
    assert torch.equal(ya, outs["nchw"][0])
    assert _nrel(outs["nchw"][1], xa.grad.to(F64)) < (2.0 ** -7 if dtype == BF16 else 1e-6)
