"""The kernels of csrc/token_pool.hip by the C ABI against tests/token_pool_ref.py in fp64, the operator and the MViT modules
over them.

Inputs are rounded to the storage type first; every buffer a kernel writes is pre-filled with a quiet NaN no kernel produces
(int8: a code no tap has), with margins in front and behind: nothing outside the outputs is written and every output element
is.  Each stage is compared with its fp64 formula on the kernel's OWN stored inputs (the LayerNorm backward on the stored
pooled rows, mean and rstd; the pool backward on the stored dpooled and indices), every element against its own bound
(token_pool_ref.py; checked without a GPU in test_token_pool_ref_cpu.py).  fp32 storage keeps the un-rounded pooled value, so
there the fused LayerNorm is also held to ln_ref's bounds on the stored rows alone.

  the case table (B = 2, both dtypes): the nine geometries of the ATen check, a strided input view, weights that do not fit
    LDS, 260 channel groups (two dw tiles), the skip pool at head_dim = C = 768, avg with the norm, and one shape whose forward
    walks its grid-stride loop twice and whose dw partials exceed one wave (both read from focus_token_pool_blocks)
  max: no ties in the inputs (asserted), values and indices exact; the tie rule on all-zero and post-ReLU maps
  two runs of the backward give the same bits
  ops.token_pool: values and the four gradients against fp64, nothing kept under torch.no_grad()
  MultiScaleAttention (pool_first or not) and MultiScaleBlock on the HIP route and forced onto the ATen route, each against an
    fp64 evaluation; the golden MViT configuration reaches ops.token_pool for every pool it has

With -s every test prints the largest error / bound of each quantity it checks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ln_ref as lr
import token_pool_ref as tr
from test_gpu_batchnorm import Buf, _ratio, _report
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

F32, BF16, F64, I8 = torch.float32, torch.bfloat16, torch.float64, torch.int8
OK = 0


def _lib():
    from focus_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _desc(g, mode, dtype, xrs=1):
    L = _lib()
    d = L.TokenPoolDesc()
    d.B, d.T, d.H, d.W, d.C, d.head_dim, d.cls = g.B, g.thw[0], g.thw[1], g.thw[2], g.C, g.hd, g.cls
    for i in range(3):
        d.k[i], d.s[i], d.p[i] = g.k[i], g.s[i], g.p[i]
    d.mode, d.dtype = mode, L.BF16 if dtype == BF16 else L.F32
    d.x_row_stride, d.x_batch_stride = xrs * g.C, g.rows_in * xrs * g.C
    return d


def _lib_blocks(g, stage):
    return _lib().lib().focus_token_pool_blocks(ctypes.byref(_desc(g, tr.CONV, F32)), stage)


_BIG = []


def _cases():
    return list(range(len(tr.CASES))) + ["big"]


def _case(i):
    if i != "big":
        return tr.CASES[i]
    if not _BIG:
        c = tr.big_case(_lib_blocks)
        g = tr.geo_of(c)
        assert tr.fwd_lanes(g, True) > _lib_blocks(g, 1) * tr.THREADS and _lib_blocks(g, 3) > 64
        _BIG.append(c)
    return _BIG[0]


def _embed(x, xrs):
    """x [B, N, C] as the middle column block of a [B, N, xrs * C] matrix filled with NaN."""
    if xrs == 1:
        return x
    B, N, C = x.shape
    wide = torch.full((B, N, xrs * C), float("nan"), dtype=x.dtype, device=x.device)
    wide[:, :, C:2 * C] = x
    return wide[:, :, C:2 * C]


def _run(c, dtype, t, d_):
    """One forward and one backward by the C ABI -> dict of the stored outputs (tensors in their own shapes)."""
    L = _lib().lib()
    g = tr.geo_of(c)
    mode = tr.MODES[c["mode"]]
    d = _desc(g, mode, dtype, c["xrs"])
    for stage in range(4):
        if not (stage == 1 and g.hd > 128):
            assert L.focus_token_pool_blocks(ctypes.byref(d), stage) == tr.blocks(g, stage)
    n_out, n_in, heads = g.B * g.rows_out * g.C, g.B * g.rows_in * g.C, g.heads
    x = _embed(t["x"], c["xrs"])
    w = t["w"].contiguous() if mode == tr.CONV else None
    y, pooled, idx = Buf(n_out, dtype, d_), Buf(n_out, dtype, d_), Buf(n_out, I8, d_)
    mean, rstd = Buf(g.B * g.rows_out * heads, F32, d_), Buf(g.B * g.rows_out * heads, F32, d_)
    norm = c["norm"]
    rc = L.focus_token_pool_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr() if w is not None else None,
                                t["gamma"].data_ptr() if norm else None, t["beta"].data_ptr() if norm else None, tr.EPS, y.ptr(),
                                pooled.ptr() if norm else None, mean.ptr() if norm else None, rstd.ptr() if norm else None,
                                idx.ptr() if mode == tr.MAX else None, _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    y.check("y"), pooled.check("pooled", written=norm), mean.check("mean", written=norm), rstd.check("rstd", written=norm)
    idx.check("idx", written=mode == tr.MAX)
    shp = (g.B, g.rows_out, g.C)
    out = dict(y=y.data().view(shp), pooled=(pooled if norm else y).data().view(shp), idx=idx.data().view(shp) if mode == tr.MAX else None,
               mean=mean.data(), rstd=rstd.data())
    # backward: the LayerNorm's existing kernel on the [B*rows*heads, head_dim] view, then the pool's
    dp = t["dy"]
    if norm:
        rows = g.B * g.rows_out * heads
        dpb, dg, db = Buf(n_out, dtype, d_), Buf(g.hd, F32, d_), Buf(g.hd, F32, d_)
        partial = torch.empty(2, L.focus_layernorm_bwd_blocks(rows), g.hd, device=d_, dtype=F32)
        rc = L.focus_layernorm_bwd(t["dy"].data_ptr(), pooled.ptr(), t["gamma"].data_ptr(), mean.ptr(), rstd.ptr(), None, dpb.ptr(),
                                   dg.ptr(), db.ptr(), partial.data_ptr(), rows, g.hd, d.dtype, _stream())
        torch.cuda.synchronize()
        assert rc == OK, rc
        dpb.check("dpooled"), dg.check("dgamma"), db.check("dbeta")
        dp = dpb.data().view(shp)
        out.update(dgamma=dg.data(), dbeta=db.data())
    out["dp"] = dp
    nbytes = L.focus_token_pool_workspace_bytes(ctypes.byref(d))
    assert nbytes == (tr.workspace_bytes(g) if mode == tr.CONV else 0)
    for rep in range(2):
        dx, dw, ws = Buf(n_in, dtype, d_), Buf(g.hd * g.K, F32, d_), Buf(max(nbytes, 16) // 4, F32, d_)
        rc = L.focus_token_pool_bwd(ctypes.byref(d), dp.data_ptr(), x.data_ptr(), w.data_ptr() if w is not None else None,
                                    idx.ptr() if mode == tr.MAX else None, dx.ptr(), dw.ptr() if mode == tr.CONV else None,
                                    ws.ptr() if mode == tr.CONV else None, nbytes, _stream())
        torch.cuda.synchronize()
        assert rc == OK, rc
        dx.check("dx"), dw.check("dw", written=mode == tr.CONV), ws.check("workspace", written=None)
        if rep == 0:
            out.update(dx=dx.data().view(g.B, g.rows_in, g.C), dw=dw.data().view(g.hd, g.K))
        else:   # the same inputs, the same bits
            assert torch.equal(out["dx"].view(torch.int16 if dtype == BF16 else torch.int32), dx.data().view(torch.int16 if dtype == BF16 else torch.int32).view(out["dx"].shape))
            if mode == tr.CONV:
                assert torch.equal(out["dw"].view(torch.int32), dw.data().view(torch.int32).view(g.hd, g.K)), "dw is not bit-repeatable"
    if c["xrs"] > 1:
        assert bool(torch.isnan(x._base[:, :, :g.C]).all()) and bool(torch.isnan(x._base[:, :, 2 * g.C:]).all())
    return out


def _check(c, dtype, t, o):
    """Every stage against fp64 on the kernel's own stored inputs -> {quantity: largest error / bound}."""
    g = tr.geo_of(c)
    bf = dtype == BF16
    mode = tr.MODES[c["mode"]]
    ref, idx, scale = tr.pool_fwd(t["x"], g, mode, t["w"])
    e, b = tr.pool_fwd_bound(g, scale, ref, bf, mode)
    r = dict(pooled=_ratio(o["pooled"], ref, b))
    if mode == tr.MAX:
        assert torch.equal(o["pooled"].to(F64), ref) and torch.equal(o["idx"], idx), "max: values and indices are exact"
    if c["norm"]:
        y, mean, rstd = tr.norm_fwd(ref, g, t["gamma"], t["beta"], tr.EPS)
        by, bm, br = tr.norm_fwd_bounds(ref, e, g, t["gamma"], t["beta"], tr.EPS, bf)
        r.update(y=_ratio(o["y"], y, by), mean=_ratio(o["mean"], mean, bm), rstd=_ratio(o["rstd"], rstd, br))
        p2 = o["pooled"].reshape(-1, g.hd)
        if not bf:       # fp32 rows are the values the kernel normalised: ln_ref's bounds on the stored rows alone
            y2, m2, r2 = lr.fwd(p2, t["gamma"], t["beta"], tr.EPS)
            bm2, br2, by2 = lr.fwd_bounds(p2, t["gamma"], t["beta"], tr.EPS, False)
            r.update(ln_y=_ratio(o["y"].reshape(-1, g.hd), y2, by2), ln_mean=_ratio(o["mean"], m2, bm2), ln_rstd=_ratio(o["rstd"], r2, br2))
        dy2 = t["dy"].reshape(-1, g.hd)
        dp_ref, dg_ref, db_ref = lr.bwd(dy2, p2, t["gamma"], o["mean"], o["rstd"])
        rows = p2.shape[0]
        sg, sb = lr.col_scale(dy2, p2, o["mean"], o["rstd"])
        k = (rows + lr.bwd_blocks(rows) + 16) * lr.U
        r.update(dpooled=_ratio(o["dp"].reshape(-1, g.hd), dp_ref, lr.bwd_bounds(dy2, p2, t["gamma"], o["mean"], o["rstd"], None, bf)),
                 dgamma=_ratio(o["dgamma"], dg_ref, k * sg), dbeta=_ratio(o["dbeta"], db_ref, k * sb))
    else:
        assert o["y"] is o["pooled"] or torch.equal(o["y"], o["pooled"])
    dx_ref, sc = tr.pool_dx(o["dp"], g, mode, t["w"], o["idx"])
    r["dx"] = _ratio(o["dx"], dx_ref, tr.pool_dx_bound(g, sc, dx_ref, bf, mode))
    if g.cls:
        assert torch.equal(o["dx"][:, 0], o["dp"][:, 0]), "the cls row of dx is dpooled row 0"
    if mode == tr.CONV:
        dw_ref, sw = tr.pool_dw(o["dp"], t["x"], g)
        r["dw"] = _ratio(o["dw"], dw_ref, tr.pool_dw_bound(g, sw))
    return r


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ci", _cases(), ids=lambda i: "big" if i == "big" else tr.case_id(tr.CASES[i]))
def test_kernels_by_the_c_abi(ci, dtype):
    d_ = dev()
    c = _case(ci)
    g = tr.geo_of(c)
    t = tr.inputs(c, dtype, seed=11, device=d_)
    keep = {k: v.clone() for k, v in t.items()}
    if c["mode"] == "max":
        assert tr.window_ties(t["x"], g) == 0
    o = _run(c, dtype, t, d_)
    for k, v in t.items():
        assert torch.equal(v, keep[k]), "input %s was written" % k
    _report("%s %s (fwd %d, dx %d, dw %d blocks)" % (tr.case_id(c), dtype, tr.blocks(g, int(c["norm"])), tr.blocks(g, 2), tr.blocks(g, 3)),
            _check(c, dtype, t, o))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_max_tie_rule(dtype):
    """All-zero and post-ReLU maps: the index, and with it the gradient, goes to the first in-bounds cell in (t, h, w) order; a
    padded tap never wins with a 0."""
    d_ = dev()
    gen = torch.Generator().manual_seed(12)
    for ci in (5, 6):
        c = tr.CASES[ci]
        g = tr.geo_of(c)
        maps = [torch.zeros(g.B, g.rows_in, g.C), (torch.randn(g.B, g.rows_in, g.C, generator=gen) - 1).clamp_min(0),
                -torch.rand(g.B, g.rows_in, g.C, generator=gen) - 1.0]
        for n, x in enumerate(maps):
            t = dict(x=x.to(dtype).to(d_), w=None, dy=torch.randn(g.B, g.rows_out, g.C, generator=gen).to(dtype).to(d_))
            if n < 2:
                assert tr.window_ties(t["x"], g) > 0
            o = _run(c, dtype, t, d_)
            ref, idx, _ = tr.pool_fwd(t["x"], g, tr.MAX)
            assert torch.equal(o["pooled"].to(F64), ref) and torch.equal(o["idx"], idx)
            if n < 2:
                assert not torch.equal(o["idx"], tr.pool_fwd(t["x"], g, tr.MAX, last=True)[1])
            else:
                assert float(o["pooled"][:, g.cls:].float().max()) < 0
            dx_ref, sc = tr.pool_dx(t["dy"], g, tr.MAX, None, idx)
            assert _ratio(o["dx"], dx_ref, tr.pool_dx_bound(g, sc, dx_ref, dtype == BF16, tr.MAX)) <= 1.0
            if n == 0:    # all zero: the gradient of a window lands on its first in-bounds cell
                first = tr.Geo.window(g, d_)
                cells, inb = first
                k0 = inb.to(torch.int8).argmax(0)                                       # the first in-bounds tap of each window
                hit = torch.zeros(g.L, dtype=torch.bool, device=d_)
                hit[cells[k0, torch.arange(g.OL, device=d_)]] = True
                ones = dict(t, dy=torch.ones_like(t["dy"]))
                dx1 = _run(c, dtype, ones, d_)["dx"]
                assert torch.equal(dx1[0, g.cls:, 0] != 0, hit)


def _nrel(a, b):
    return float((a.to(F64) - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ci", [0, 1, 5, 7, 9], ids=lambda i: tr.case_id(tr.CASES[i]))
def test_ops_token_pool_against_fp64(ci, dtype):
    """ops.token_pool against the fp64 chain.  The output is held element by element to the bounds of the forward stages.  The
    operator's stored intermediates (pooled rows, mean, rstd, dpooled) are not visible here, so the gradients of x, weight, gamma
    and beta cannot be checked stage by stage on stored inputs as test_kernels_by_the_c_abi does; they are held norm-wise to
    the suite's parity bound, 1e-3 relative in fp32, and to 2^-7 in bf16: two bf16 roundings of a stored intermediate (pooled
    rows, dpooled) at 2^-8 each on the way to any gradient.  Under torch.no_grad() nothing is kept."""
    from focus_amd import ops
    d_ = dev()
    c = tr.CASES[ci]
    g = tr.geo_of(c)
    mode = tr.MODES[c["mode"]]
    t = tr.inputs(c, dtype, seed=13, device=d_)
    x = _embed(t["x"], c["xrs"]).detach().requires_grad_()
    w = t["w"].clone().requires_grad_() if mode == tr.CONV else None
    gamma, beta = t["gamma"].clone().requires_grad_(), t["beta"].clone().requires_grad_()
    norm = (gamma, beta, tr.EPS) if c["norm"] else None
    assert ops.token_pool_ok(x, g.hd, c["mode"], g.k, g.s, g.p, norm, w)
    y, thw = ops.token_pool(x, g.thw, c["mode"], w, g.k, g.s, g.p, bool(g.cls), g.hd, norm)
    assert list(thw) == list(g.out) and y.dtype == dtype and tuple(y.shape) == (g.B, g.rows_out, g.C)
    y.backward(t["dy"])
    ref, idx, scale = tr.pool_fwd(t["x"], g, mode, t["w"])
    e, b = tr.pool_fwd_bound(g, scale, ref, dtype == BF16, mode)
    dp = t["dy"].to(F64)
    r = {}
    tol = 1e-3 if dtype == F32 else 2.0 ** -7
    if c["norm"]:
        yr, mean, rstd = tr.norm_fwd(ref, g, t["gamma"], t["beta"], tr.EPS)
        r["y"] = _ratio(y.detach(), yr, tr.norm_fwd_bounds(ref, e, g, t["gamma"], t["beta"], tr.EPS, dtype == BF16)[0])
        d2, dg, db = lr.bwd(t["dy"].reshape(-1, g.hd), ref.reshape(-1, g.hd), t["gamma"], mean, rstd)
        dp = d2.reshape(ref.shape)
        r["dgamma"], r["dbeta"] = _nrel(gamma.grad, dg) / tol, _nrel(beta.grad, db) / tol
    else:
        r["y"] = _ratio(y.detach(), ref, b)
        assert gamma.grad is None
    dx_ref, _ = tr.pool_dx(dp, g, mode, t["w"], idx)
    r["dx"] = _nrel(x.grad, dx_ref) / tol
    assert x.grad.dtype == dtype and tuple(x.grad.shape) == tuple(x.shape)
    if mode == tr.CONV:
        dw_ref, _ = tr.pool_dw(dp, t["x"], g)
        assert w.grad.dtype == F32 and w.grad.shape == w.shape
        r["dw"] = _nrel(w.grad.reshape(g.hd, g.K), dw_ref) / tol
    _report("ops.token_pool %s %s" % (tr.case_id(c), dtype), r)
    # nothing is kept without a tape: no grad_fn, no saved tensor, and only y (and the int8 indices' storage freed) allocated
    packed = []
    with torch.no_grad(), torch.autograd.graph.saved_tensors_hooks(lambda v: packed.append(v) or v, lambda v: v):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y2, _ = ops.token_pool(x, g.thw, c["mode"], w, g.k, g.s, g.p, bool(g.cls), g.hd, norm)
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - before
    assert y2.grad_fn is None and not packed and torch.equal(y2, y.detach())
    assert grown <= y2.numel() * y2.element_size() + 4096, "a forward under no_grad keeps more than its output"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_pool(t["x"].cpu(), g.thw, c["mode"], None if w is None else w.detach().cpu(), g.k, g.s, g.p, bool(g.cls), g.hd, None)


# ---- the modules ------------------------------------------------------------------------------------------------------------
def _attn64(sd, x, thw, heads, pool_first, prefix=""):
    """MultiScaleAttention (conv mode, cls) in fp64 from a state dict."""
    p = lambda n: sd[prefix + n].to(F64)
    B, N, C = x.shape
    hd = C // heads
    lin = lambda t, n: F.linear(t, p(n + ".weight"), p(n + ".bias") if prefix + n + ".bias" in sd else None)
    out = {}
    for n in ("q", "k", "v"):
        t = x if pool_first else lin(x, n)
        w = p("pool_%s.weight" % n)
        k = tuple(w.shape[2:])
        s = sd["_stride_" + n]
        g = tr.Geo(B, thw, k, s, heads, hd, 1)
        t = tr.aten_pool(t, g, tr.CONV, w, (p("norm_%s.weight" % n), p("norm_%s.bias" % n), sd["_eps"]))
        out[n] = (lin(t, n) if pool_first else t, list(g.out))
    h = lambda t: t.reshape(B, -1, heads, hd).transpose(1, 2)
    a = torch.softmax(h(out["q"][0]) * hd ** -0.5 @ h(out["k"][0]).transpose(-1, -2), -1) @ h(out["v"][0])
    return lin(a.transpose(1, 2).reshape(B, -1, C), "proj"), out["q"][1]


def _block64(sd, x, thw, heads, dim_out):
    p = lambda n: sd[n].to(F64)
    C = x.shape[-1]
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), p(n + ".weight"), p(n + ".bias"), sd["_eps_block"])
    xb, thw_new = _attn64(sd, ln(x, "norm1"), thw, heads, False, "attn.")
    g = tr.Geo(x.shape[0], thw, sd["_skip_k"], sd["_stride_q"], 1, C, 1)
    x = tr.aten_pool(x, g, tr.MAX) + xb
    xn = ln(x, "norm2")
    if C != dim_out:
        x = F.linear(xn, p("proj.weight"), p("proj.bias"))
    return x + F.linear(F.gelu(F.linear(xn, p("mlp.fc1.weight"), p("mlp.fc1.bias"))), p("mlp.fc2.weight"), p("mlp.fc2.bias")), thw_new


def _module_pair(make, d_):
    torch.manual_seed(21)
    a = make().to(d_)
    for n, q in a.named_parameters():
        if "norm" in n and n.endswith("weight"):
            q.data.add_(0.2 * torch.randn_like(q))
        elif n.endswith("bias"):
            q.data.add_(0.1 * torch.randn_like(q))
    b = make().to(d_)
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", ["attention", "attention-pool-first", "block"])
def test_modules_on_both_routes_against_fp64(which, dtype, monkeypatch):
    """The module built twice from one state dict: one copy on the HIP route, one forced onto the ATen route (token_pool_ok
    patched to refuse), output and every parameter gradient of both against an fp64 evaluation on the CPU.  The two routes are
    not compared with each other: in bf16 the ATen route rounds the pooled value before its LayerNorm and the HIP route does
    not.  Bound: the parity bounds of this suite for a composed module (tests/test_gpu_parity.py TOL: 1e-3 norm-wise relative in
    fp32, 3e-2 in bf16, where every stored activation of the chain is rounded to 8 bits)."""
    from focus_amd import ops
    from focus_amd.slowfast.models import attention as A
    d_ = dev()
    heads, C, thw = 2, 32, [2, 6, 6]
    kw = dict(kernel_q=(3, 3, 3), kernel_kv=(3, 3, 3), stride_q=(1, 2, 2), stride_kv=(1, 2, 2))
    if which == "block":
        make = lambda: A.MultiScaleBlock(C, 2 * C, heads, **kw)
    else:
        make = lambda: A.MultiScaleAttention(C, num_heads=heads, pool_first=which.endswith("first"), **kw)
    hip, aten = _module_pair(make, d_)
    gen = torch.Generator().manual_seed(22)
    x0 = torch.randn(2, 1 + 72, C, generator=gen).to(dtype)
    n_out = 2 * C if which == "block" else C
    ct = torch.randn(2, 1 + 18, n_out, generator=gen).to(dtype)
    sd = {k: v.detach().cpu() for k, v in hip.state_dict().items()}
    params64 = {k: v.to(F64).requires_grad_() for k, v in sd.items()}
    extra = dict(_stride_q=(1, 2, 2), _stride_k=(1, 2, 2), _stride_v=(1, 2, 2), _eps=1e-5, _eps_block=1e-5, _skip_k=(1, 3, 3))
    x64 = x0.to(F64).requires_grad_()
    y64, thw64 = (_block64({**params64, **extra}, x64, thw, heads, 2 * C) if which == "block"
                  else _attn64({**params64, **extra}, x64, thw, heads, which.endswith("first")))
    (y64 * ct.to(F64)).sum().backward()
    tol = 1e-3 if dtype == F32 else 3e-2
    calls = []
    real = ops.token_pool
    monkeypatch.setattr(ops, "token_pool", lambda *a, **k: calls.append(a[2]) or real(*a, **k))
    for name, m in (("hip", hip), ("aten", aten)):
        if name == "aten":
            monkeypatch.setattr(ops, "token_pool_ok", lambda *a, **k: False)
        calls.clear()
        x = x0.to(d_).requires_grad_()
        y, shape = m(x, None, thw) if which == "block" else m(x, thw)
        assert list(shape) == thw64 == [2, 3, 3]
        (y.float() * ct.to(d_).float()).sum().backward()
        assert calls == ((["conv"] * 3 + (["max"] if which == "block" else [])) if name == "hip" else [])
        r = dict(y=_nrel(y.detach().cpu(), y64.detach()) / tol, dx=_nrel(x.grad.cpu(), x64.grad) / tol)
        for k, q in m.named_parameters():
            assert q.grad is not None, k
            ref = params64[k].grad
            # norm_k.bias shifts every logit of a query by the same amount: its exact gradient is 0, and the error is
            # measured against the gradient of norm_k.weight, which the same sums form
            scale = (params64[k.replace("bias", "weight")].grad if k.endswith("norm_k.bias") else ref).norm()
            r[k] = float((q.grad.cpu().to(F64) - ref).norm() / scale) / (tol * (3 if dtype == BF16 else 1))
        _report("%s %s %s" % (which, name, dtype), r)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_the_golden_mvit_reaches_the_hip_op_for_every_pool(dtype, monkeypatch):
    from conftest import load_golden
    from focus_amd import ops
    from focus_amd.slowfast.models import attention as A
    from focus_amd.slowfast.models import build_model
    from test_gpu_parity import T, _mvit_small_cfg
    a, p = load_golden("mvit_orvit_small")
    m = build_model(_mvit_small_cfg(dtype == BF16))
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    m.train()
    pools = [q for blk in m.modules() if isinstance(blk, A.MultiScaleBlock)
             for q in (blk.attn.pool_q, blk.attn.pool_k, blk.attn.pool_v, blk.pool_skip) if q is not None]
    assert len(pools) >= 4
    seen, aten = [], []
    real, real_pool = ops.token_pool, A.attention_pool
    monkeypatch.setattr(ops, "token_pool", lambda *a_, **k: seen.append(a_[2]) or real(*a_, **k))
    monkeypatch.setattr(A, "attention_pool", lambda t, pool, *a_, **k: aten.append(pool) or real_pool(t, pool, *a_, **k))
    y = m([T(a["x"]).float().to(dev())], {"orvit_bboxes": T(a["boxes"]).to(dev())})
    assert bool(torch.isfinite(y.float()).all())
    assert len(seen) == len(pools) and not aten
    assert sorted(seen) == sorted("conv" if isinstance(q, torch.nn.Conv3d) else "max" for q in pools)
