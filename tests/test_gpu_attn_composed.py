"""The composed route of ops.small_attention and the row-softmax kernels under it (csrc/softmax.hip).

a. focus_softmax_fwd / focus_softmax_causal_fwd / focus_softmax_bwd by the C ABI against tests/attn_ref.py in fp64 on
   the same rounded inputs: lengths around the 64 lanes of a wave, row counts around the 4 rows of a block, padded row
   strides with every bit outside the rows pinned, in place and out of place, the causal tail, status codes, repeatability.
b. ops.small_attention wherever it does not take the one-launch kernels (_SmallAttnFn: six strided batched GEMMs around
   those softmax kernels), over attn_ref.CASES: the route, out / dq / dk / dv against the formula, the exact consequences
   of the causal mask, repeatability.  The table and its conditioning are checked without a GPU in test_attn_ref_cpu.py.

The error table of part b as measured on an MI355X is the comment at the end of this file."""
import ctypes

import pytest
import torch

import attn_ref as ar
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
OK, ERR_SHAPE, ERR_NULL = 0, -1, -5
NAN_BITS = {F32: 0x7FC00123, BF16: 0x7FC1}       # the pre-fill of every output buffer: a quiet NaN no kernel produces
FRONT, TAIL = 8, 64                              # elements in front of the first row and behind the last one

# ---- bounds of part a, derived (u = 2^-24, the fp32 unit roundoff; A = max |scale * x| over the visible row) ----------
# forward, fp32 arithmetic on exact inputs:
#   t = scale * x            one rounding, |dt| <= u A                      (the row maximum m is one of the t: same value)
#   a = t - m                one rounding of a value of size <= 2A, |da| <= 2u A
#   __expf(a) = exp2(a * log2(e)): the product is rounded, an error of u |a log2 e| in the exponent = ln2 * that =
#                            u |a| <= 2u A relative in the result; log2(e) itself is off by <= 2^-25 relative: u A more;
#                            v_exp_f32 is good to 1 ulp = 2u
#   so every exponential is off by at most E = (6 A + 2) u relative (A ~ 140 at randn * 30: 5e-5, the "about 1e-5" of a
#   rounding at magnitude 200).  The sum of L positive terms, 64 partial sums and a 6-step butterfly: <= (L / 64 + 7) u
#   relative, bounded here by (L + 7) u; 1 / s and the product with it: 2 ulp + 1 rounding <= 5u.  With the errors of the
#   numerator and of the sum:   |dy| <= (2 E + (L + 12) u) * y = REL(A, L) * y.
#   Below the normal range (exp of less than -87) the hardware may flush: an absolute 2^-125 on top.
# bf16 output: one more round to nearest (f32_to_bf16), 2^-8 * y elementwise.
# an fp32 row sums to 1 within REL plus the L roundings of the stored values, L u.
U = 2.0 ** -24
TINY = 2.0 ** -125


def fwd_rel(A, L):
    return (2 * (6 * A + 2) + L + 12) * U


# backward, per row, relative to ref = |scale| * max|y| * (max|dy| + |sum(dy * y)|): L fp32 ulps (2^-23) of it -- the L
# products and additions of the sum and the four operations after it -- plus 2^-8 of it for a bf16 result.
ULP = 2.0 ** -23


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _nan_buffer(n, dtype, d):
    return torch.full((n,), NAN_BITS[dtype], device=d, dtype=torch.int16 if dtype == BF16 else torch.int32).view(dtype)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(buf, off=FRONT):
    return buf.data_ptr() + off * buf.element_size()


def _dt(dtype):
    from focus_amd import _lib
    return _lib.BF16 if dtype == BF16 else _lib.F32


def _rows_view(buf, rows, L, stride):
    return torch.as_strided(buf, (rows, L), (stride, 1), FRONT)


def _place(vals, stride, dtype, d):
    """vals [rows, L] (CPU, already rounded) laid out with `stride` in a NaN-filled buffer with margins."""
    rows, L = vals.shape
    buf = _nan_buffer(FRONT + rows * stride + TAIL, dtype, d)
    _rows_view(buf, rows, L, stride).copy_(vals.to(d))
    return buf


def _outside_untouched(buf, rows, L, stride, what):
    """Every bit outside [row * stride, row * stride + L) still is the pre-fill, the space after the last row included."""
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    _rows_view(keep, rows, L, stride).fill_(False)
    assert int(keep.sum()) == buf.numel() - rows * L
    nan = NAN_BITS[buf.dtype]
    assert bool((_bits(buf)[keep] == nan).all()), what + ": written outside the rows"


def _softmax_fwd(x, y, rows, L, stride, scale, dtype, period=None):
    from focus_amd import _lib
    lib = _lib.lib()
    if period is None:
        rc = lib.focus_softmax_fwd(_ptr(x), _ptr(y), rows, L, stride, scale, _dt(dtype), _stream())
    else:
        rc = lib.focus_softmax_causal_fwd(_ptr(x), _ptr(y), rows, L, stride, period, scale, _dt(dtype), _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc


def _softmax_bwd(dy, y, dx, rows, L, stride, scale, dtype):
    from focus_amd import _lib
    rc = _lib.lib().focus_softmax_bwd(_ptr(dy), _ptr(y), _ptr(dx), rows, L, stride, scale, _dt(dtype), _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc


def _values(rows, L, s, dtype, g):
    x = torch.randn(rows, L, generator=g) * s
    if rows > 1:
        x[rows // 2] = 3.25                                # one row of all-equal values: exactly uniform in fp64
    return x.to(dtype)


def _check_fwd(got, x, scale, dtype, period, what):
    """got, x: [rows, L] on the CPU; x in the dtype."""
    rows, L = x.shape
    want = ar.softmax_rows(x, scale, period)
    z = (scale * x.double()).abs()
    if period is not None:
        hidden = torch.arange(L)[None, :] > (torch.arange(rows) % period)[:, None]
        z = z.masked_fill(hidden, 0.0)
        assert bool((_bits(got)[hidden] == 0).all()), what + ": the masked tail is not +0.0"
    rel = fwd_rel(z.max(-1, keepdim=True).values, L)
    bound = rel * want + TINY + (2.0 ** -8 * want if dtype == BF16 else 0.0)
    e = (got.double() - want).abs()
    assert torch.isfinite(got.float()).all(), what
    worst = float((e / bound).max())
    assert worst <= 1.0, "%s: %.3f of the bound (REL up to %.2e)" % (what, worst, float(rel.max()))
    if dtype == F32:
        off = (got.double().sum(-1, keepdim=True) - 1.0).abs()
        assert bool((off <= rel + L * U).all()), "%s: a row sums to 1 %+.3e" % (what, float(off.max()))
    return worst


SHAPES = [  # rows, L: every L and every row count of the issue, crossed thinly
    (1, 1), (3, 2), (5, 63), (1023, 64), (3, 65), (5, 127), (1, 129), (1023, 197), (5, 1024), (3, 1025),
    (1023, 1), (5, 2), (1, 64), (5, 65), (3, 129), (1, 1025),
]
_f32 = lambda a: float(torch.tensor(a, dtype=torch.float32))     # the scale crosses the ABI as a float: the reference gets that value
VALUES = [(1.0, 1.0), (30.0, 1.0), (1.0, _f32(48 ** -0.5)), (30.0, -0.5), (30.0, _f32(48 ** -0.5))]     # s of randn * s, scale


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,L", SHAPES)
def test_softmax_fwd_values_window_in_place_repeat(rows, L, dtype):
    d = dev()
    g = torch.Generator().manual_seed(1000 * rows + L)
    for pad in (0, 3):
        stride = L + pad
        for s, scale in VALUES:
            what = "rows %d L %d stride %d randn * %g scale %g" % (rows, L, stride, s, scale)
            x = _values(rows, L, s, dtype, g)
            xb = _place(x, stride, dtype, d)
            x0 = xb.clone()
            y1, y2 = _nan_buffer(xb.numel(), dtype, d), _nan_buffer(xb.numel(), dtype, d)
            _softmax_fwd(xb, y1, rows, L, stride, scale, dtype)
            _softmax_fwd(xb, y2, rows, L, stride, scale, dtype)
            assert torch.equal(_bits(xb), _bits(x0)), what + ": the input was written"
            _outside_untouched(y1, rows, L, stride, what)
            assert torch.equal(_bits(y1), _bits(y2)), what + ": two launches differ"
            _softmax_fwd(xb, xb, rows, L, stride, scale, dtype)                    # y is x, as ops.py calls it
            assert torch.equal(_bits(xb), _bits(y1)), what + ": in place differs from out of place"
            _check_fwd(_rows_view(y1, rows, L, stride).cpu(), x, scale, dtype, None, what)


CAUSAL = [(1, 1), (5, 5), (11, 11), (64, 64), (65, 65), (11, 14), (11, 7)]     # period, L


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("period,L", CAUSAL)
def test_softmax_causal_fwd_and_its_backward(period, L, dtype):
    """rows = 6 * period: blocks of four rows straddle sequence ends.  The masked columns of the input hold 1e30 (the GEMM in
    front writes finite garbage there); they must reach neither the maximum nor the sum, and come out as +0.0."""
    d = dev()
    rows = 6 * period
    g = torch.Generator().manual_seed(77 * period + L)
    hidden = torch.arange(L)[None, :] > (torch.arange(rows) % period)[:, None]
    for pad in (0, 3):
        stride = L + pad
        for s, scale in VALUES:
            what = "period %d L %d stride %d randn * %g scale %g" % (period, L, stride, s, scale)
            x = _values(rows, L, s, dtype, g)
            x[hidden] = 1e30
            xb = _place(x, stride, dtype, d)
            y1, y2 = _nan_buffer(xb.numel(), dtype, d), _nan_buffer(xb.numel(), dtype, d)
            _softmax_fwd(xb, y1, rows, L, stride, scale, dtype, period)
            _softmax_fwd(xb, y2, rows, L, stride, scale, dtype, period)
            _outside_untouched(y1, rows, L, stride, what)
            assert torch.equal(_bits(y1), _bits(y2)), what + ": two launches differ"
            _softmax_fwd(xb, xb, rows, L, stride, scale, dtype, period)
            assert torch.equal(_bits(xb), _bits(y1)), what + ": in place differs from out of place"
            y = _rows_view(y1, rows, L, stride).cpu()
            _check_fwd(y, x, scale, dtype, period, what)
            # the backward of the causal rows is the plain one: y = 0 makes dx = 0 whatever dy holds there
            dy = torch.randn(rows, L, generator=g).to(dtype)
            dyb = _place(dy, stride, dtype, d)
            dx = _nan_buffer(dyb.numel(), dtype, d)
            _softmax_bwd(dyb, y1, dx, rows, L, stride, scale, dtype)
            _outside_untouched(dx, rows, L, stride, what + " bwd")
            got = _rows_view(dx, rows, L, stride).cpu()
            assert bool((got[hidden] == 0).all()), what + ": dx is not zero under the mask"
            _check_bwd(got, dy, y, scale, dtype, what)


def _check_bwd(got, dy, y, scale, dtype, what):
    L = y.shape[-1]
    want = ar.softmax_rows_bwd(dy, y, scale)
    dyd, yd = dy.double(), y.double()
    ref = abs(scale) * yd.abs().max(-1, keepdim=True).values * (
        dyd.abs().max(-1, keepdim=True).values + (dyd * yd).sum(-1, keepdim=True).abs())
    bound = (L * ULP + (2.0 ** -8 if dtype == BF16 else 0.0)) * ref + TINY
    assert torch.isfinite(got.float()).all(), what
    worst = float(((got.double() - want).abs() / bound).max())
    assert worst <= 1.0, "%s bwd: %.3f of the bound" % (what, worst)
    return worst


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,L", SHAPES)
def test_softmax_bwd_values_window_in_place_repeat(rows, L, dtype):
    d = dev()
    g = torch.Generator().manual_seed(2000 * rows + L)
    for pad in (0, 3):
        stride = L + pad
        for s, scale in VALUES:
            what = "rows %d L %d stride %d randn * %g scale %g" % (rows, L, stride, s, scale)
            y = ar.softmax_rows(_values(rows, L, s, dtype, g), scale).to(dtype)
            dy = torch.randn(rows, L, generator=g).to(dtype)
            yb, dyb = _place(y, stride, dtype, d), _place(dy, stride, dtype, d)
            y0, dy0 = yb.clone(), dyb.clone()
            d1, d2 = _nan_buffer(yb.numel(), dtype, d), _nan_buffer(yb.numel(), dtype, d)
            _softmax_bwd(dyb, yb, d1, rows, L, stride, scale, dtype)
            _softmax_bwd(dyb, yb, d2, rows, L, stride, scale, dtype)
            assert torch.equal(_bits(yb), _bits(y0)) and torch.equal(_bits(dyb), _bits(dy0)), what + ": an input was written"
            _outside_untouched(d1, rows, L, stride, what)
            assert torch.equal(_bits(d1), _bits(d2)), what + ": two launches differ"
            _softmax_bwd(dyb, yb, dyb, rows, L, stride, scale, dtype)              # dx is dy, as ops.py and traj_attn.hip call it
            assert torch.equal(_bits(dyb), _bits(d1)), what + ": in place differs from out of place"
            assert torch.equal(_bits(yb), _bits(y0)), what + ": y was written"
            _check_bwd(_rows_view(d1, rows, L, stride).cpu(), dy, y, scale, dtype, what)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_softmax_status_codes_leave_the_output_alone(dtype):
    """Only arguments the entry points reject or ignore before any launch."""
    from focus_amd import _lib
    lib = _lib.lib()
    d = dev()
    rows, L = 5, 7
    x = _place(torch.ones(rows, L).to(dtype), L, dtype, d)
    dt, st = _dt(dtype), _stream()
    calls = [
        ("fwd x null", lambda y: lib.focus_softmax_fwd(None, _ptr(y), rows, L, L, 1.0, dt, st), ERR_NULL),
        ("fwd rows 0", lambda y: lib.focus_softmax_fwd(_ptr(x), _ptr(y), 0, L, L, 1.0, dt, st), OK),
        ("fwd L 0", lambda y: lib.focus_softmax_fwd(_ptr(x), _ptr(y), rows, 0, L, 1.0, dt, st), OK),
        ("causal x null", lambda y: lib.focus_softmax_causal_fwd(None, _ptr(y), rows, L, L, L, 1.0, dt, st), ERR_NULL),
        ("causal period 0", lambda y: lib.focus_softmax_causal_fwd(_ptr(x), _ptr(y), rows, L, L, 0, 1.0, dt, st), ERR_SHAPE),
        ("causal period -3", lambda y: lib.focus_softmax_causal_fwd(_ptr(x), _ptr(y), rows, L, L, -3, 1.0, dt, st), ERR_SHAPE),
        ("causal rows 0", lambda y: lib.focus_softmax_causal_fwd(_ptr(x), _ptr(y), 0, L, L, L, 1.0, dt, st), OK),
        ("causal L 0", lambda y: lib.focus_softmax_causal_fwd(_ptr(x), _ptr(y), rows, 0, L, L, 1.0, dt, st), OK),
        ("bwd dy null", lambda y: lib.focus_softmax_bwd(None, _ptr(x), _ptr(y), rows, L, L, 1.0, dt, st), ERR_NULL),
        ("bwd y null", lambda y: lib.focus_softmax_bwd(_ptr(x), None, _ptr(y), rows, L, L, 1.0, dt, st), ERR_NULL),
        ("bwd rows 0", lambda y: lib.focus_softmax_bwd(_ptr(x), _ptr(x), _ptr(y), 0, L, L, 1.0, dt, st), OK),
        ("bwd L 0", lambda y: lib.focus_softmax_bwd(_ptr(x), _ptr(x), _ptr(y), rows, 0, L, 1.0, dt, st), OK),
    ]
    for what, call, want in calls:
        y = _nan_buffer(x.numel(), dtype, d)
        rc = call(y)
        torch.cuda.synchronize()
        assert rc == want, "%s: status %d, expected %d" % (what, rc, want)
        assert bool((_bits(y) == NAN_BITS[dtype]).all()), what + ": the output was written"
    # a null output: nothing to look at but the status
    assert lib.focus_softmax_fwd(_ptr(x), None, rows, L, L, 1.0, dt, st) == ERR_NULL
    assert lib.focus_softmax_causal_fwd(_ptr(x), None, rows, L, L, L, 1.0, dt, st) == ERR_NULL
    assert lib.focus_softmax_bwd(_ptr(x), _ptr(x), None, rows, L, L, 1.0, dt, st) == ERR_NULL
    torch.cuda.synchronize()


# ---- b. the composed route ------------------------------------------------------------------------------------------
NAMES = ("out", "dq", "dk", "dv")


def _counted_gemm(monkeypatch):
    from focus_amd import ops
    calls = []
    real = ops.gemm

    def counted(*a, **kw):
        calls.append(a[:3])
        return real(*a, **kw)

    monkeypatch.setattr(ops, "gemm", counted)
    return calls


def _device_inputs(case, d):
    """-> leaves (what .grad lands on), q, k, v as the route receives them, the cotangent, drop, scale; CPU originals."""
    q, k, v, cu, drop, scale = ar.inputs(case)
    C = q.shape[2]
    if case["layout"] == "qkv":
        qkv = torch.cat([q, k, v], dim=2).to(d).requires_grad_()
        qd, kd, vd = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        assert not qd.is_contiguous()
        leaves = lambda: (qkv.grad[..., :C], qkv.grad[..., C:2 * C], qkv.grad[..., 2 * C:])
    else:
        qd, kd, vd = (t.to(d).requires_grad_() for t in (q, k, v))
        leaves = lambda: (qd.grad, kd.grad, vd.grad)
    cud = cu.to(d)
    if case["layout"] == "cu_view":
        wide = torch.zeros(cu.shape[0], cu.shape[1], 2 * C, device=d, dtype=cu.dtype)
        wide[..., :C] = cud
        cud = wide[..., :C]
        assert not cud.is_contiguous()
    return leaves, qd, kd, vd, cud, None if drop is None else drop.to(d), scale


@pytest.mark.parametrize("case", ar.CASES, ids=ar.case_id)
def test_composed_route_against_the_formula(case, monkeypatch):
    from focus_amd import ops
    d = dev()
    dt, heads, causal = case["dtype"], case["heads"], case["causal"]
    Nq, Nk = case["Nq"], case["Nk"]
    leaves, q, k, v, cu, drop, scale = _device_inputs(case, d)
    calls = _counted_gemm(monkeypatch)
    out = ops.small_attention(q, k, v, heads, scale, causal=causal, drop=drop)
    assert len(calls) == 2, "the forward took %d gemm calls: not the composed route" % len(calls)
    att = out.grad_fn.saved_tensors[3]                     # the probabilities as stored, before the dropout multiplier
    out.backward(cu)
    assert len(calls) == 6, "the backward took %d gemm calls: not the composed route" % (len(calls) - 2)
    torch.cuda.synchronize()
    got = (out.detach(),) + tuple(leaves())
    for name, t in zip(NAMES, got):
        assert t.dtype == dt and torch.isfinite(t.float()).all(), name

    qx, kx, vx, cux = (t.detach().contiguous() for t in (q, k, v, cu))
    exact = ar.attention(qx, kx, vx, heads, scale, causal, drop, cux)
    model = ar.attention_rounded(qx, kx, vx, heads, scale, causal, drop, cux, dt)
    failed = []
    for name, g_, m, e in zip(NAMES, got, model, exact):
        ek, em, ekm = ar.err(g_, e), ar.err(m, e), ar.err(g_, m)
        tol = max(ar.FLOOR[dt], ar.FACTOR * em)
        assert ar.FACTOR * em <= ar.CAP[dt]
        print("%-40s %-3s err(kernel, exact) %.3e  err(model, exact) %.3e  ratio %6.3f  tol %.3e  err(kernel, model) %.3e"
              % (ar.case_id(case), name, ek, em, ek / em, tol, ekm))
        if not ek <= tol:
            failed.append("%s: %.3e > %.3e" % (name, ek, tol))
    assert not failed, "; ".join(failed)

    if causal:
        # query 0 sees key 0 only: its probability row is exactly [1, 0, 0, ...]
        first = att[:, :, 0, :].float()
        assert bool((first[..., 0] == 1).all()) and bool((_bits(att[:, :, 0, 1:].contiguous()) == 0).all())
        upper = torch.triu(torch.ones(Nq, Nk, dtype=torch.bool, device=d), diagonal=1)
        assert bool((_bits(att.contiguous())[:, :, upper] == 0).all()), "the masked probabilities are not +0.0"
        if drop is None:
            # ... so out[:, 0] is v[:, 0]: a product by 1 summed with nothing, one rounding of the dtype at most
            one = 2.0 ** -8 if dt == BF16 else 2.0 ** -23
            o0, v0 = got[0][:, 0].double(), vx[:, 0].double()
            assert bool(((o0 - v0).abs() <= one * v0.abs()).all()), "out[:, 0] is not v[:, 0]"
        # dk, dv of the last key depend on the last query only (which sees every key: no mask)
        last = lambda t: t[:, -1:]
        d1 = None if drop is None else drop[:, :, -1:]
        e1 = ar.attention(last(qx), kx, vx, heads, scale, False, d1, last(cux))
        m1 = ar.attention_rounded(last(qx), kx, vx, heads, scale, False, d1, last(cux), dt)
        for i in (2, 3):
            assert ar.err(e1[i][:, -1], exact[i][:, -1]) <= 1e-12
            ek, em = ar.err(got[i][:, -1], e1[i][:, -1]), ar.err(m1[i][:, -1], e1[i][:, -1])
            tol = max(ar.FLOOR[dt], ar.FACTOR * em)
            print("%-40s %-3s[:, Nk-1] err(kernel, exact) %.3e  err(model, exact) %.3e  tol %.3e" % (ar.case_id(case), NAMES[i], ek, em, tol))
            assert ek <= tol, "%s of the last key: %.3e > %.3e" % (NAMES[i], ek, tol)


@pytest.mark.parametrize("index", [3, 5], ids=lambda i: ar.case_id(ar.CASES[i]))
def test_composed_route_repeats_bit_for_bit(index):
    """Forward twice, and the backward twice on one graph: the in-place softmax backward works on its own copy of dA,
    never on the saved probabilities."""
    from focus_amd import ops
    case = ar.CASES[index]
    assert case["causal"]
    d = dev()
    _, q, k, v, cu, drop, scale = _device_inputs(case, d)
    out = ops.small_attention(q, k, v, case["heads"], scale, causal=True, drop=drop)
    again = ops.small_attention(q, k, v, case["heads"], scale, causal=True, drop=drop)
    assert torch.equal(_bits(out.detach()), _bits(again.detach()))
    att0 = out.grad_fn.saved_tensors[3].clone()
    leaves = (q, k, v) if case["layout"] != "qkv" else (q._base,)
    g1 = torch.autograd.grad(out, leaves, cu, retain_graph=True)
    g2 = torch.autograd.grad(out, leaves, cu, retain_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.grad_fn.saved_tensors[3]), _bits(att0)), "the backward wrote the saved probabilities"
    for a, b in zip(g1, g2):
        assert torch.equal(_bits(a), _bits(b))


# Measured on an MI355X: err(kernel, exact) / err(model, exact) for out, dq, dk, dv (largest err(kernel, exact) of the row).
#   2x4x1024x1024x48 fp32 causal          2.57   4.04  29.02  32.71   (2.0e-6)
#   2x4x1024x1024x48 fp32 causal p 0.1    1.70   2.79  20.08  26.53   (1.7e-6)
#   2x4x1024x11x48   fp32 p 0.1           2.67   3.02  15.96  22.18   (1.1e-6)
#   3x3x77x77x24     bf16 causal p 0.25   1.00   1.00   1.00   1.00   (3.6e-3)
#   2x2x5x5x96       bf16                 1.00   1.00   1.00   1.00   (4.6e-3)
#   32x4x11x11x48    fp32 causal          1.81   2.82   3.57   1.84   (2.0e-7)
#   32x4x11x11x48    bf16 p 0.1           1.00   1.00   1.00   1.00   (6.5e-3)
#   1x2x785x197x96   fp32                 9.76   8.34  22.48  17.84   (1.3e-6)
#   1x1x129x129x8    bf16 causal          1.00   1.00   1.00   1.00   (3.8e-3)
# In bf16 the kernels' error is the storage format's (err(kernel, model) is 0 to 2e-4): FACTOR = 4 is not needed there.  In
# fp32 the model's error is a few 2^-24, the sums of up to 1024 terms in dk and dv cost up to 33 times that, and every row
# stays 5 times under FLOOR = 1e-5, which is what decides the fp32 rows.  FACTOR stays at 4.
