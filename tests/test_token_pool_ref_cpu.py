"""tests/token_pool_ref.py checked without a GPU, and the host side of csrc/token_pool.hip.

  the fp64 formulas in token layout equal the ATen composition (conv3d / max_pool3d / avg_pool3d + layer_norm through the
    permutes of attention_pool): values and the gradients of x, weight, gamma, beta, at every geometry of the case table
  an fp32 twin of every stage stays inside the bounds; every mutant leaves them
  the walk of the grids equals focus_token_pool_blocks / focus_token_pool_workspace_bytes
  the descriptor's ctypes layout is the header's; every status code comes back before a launch, in the documented order
  the truth table of ops.token_pool_ok; CPU tensors keep the ATen path in the MViT modules"""
import ctypes
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ln_ref as lr
import token_pool_ref as tr

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def _close(a, b, what, tol=1e-11):
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * max(1.0, float(b.abs().max()) if b.numel() else 1.0), "%s: %g" % (what, err)


def _ref_chain(c, t, g):
    """Forward and every gradient of a case by the fp64 formulas, from inputs t."""
    mode = tr.MODES[c["mode"]]
    pooled, idx, scale = tr.pool_fwd(t["x"], g, mode, t["w"])
    out = dict(pooled=pooled, idx=idx, scale=scale)
    dp = t["dy"].to(F64)
    if c["norm"]:
        out["y"], out["mean"], out["rstd"] = tr.norm_fwd(pooled, g, t["gamma"], t["beta"], tr.EPS)
        d2, out["dgamma"], out["dbeta"] = lr.bwd(t["dy"].reshape(-1, g.hd), pooled.reshape(-1, g.hd), t["gamma"], out["mean"], out["rstd"])
        dp = d2.reshape(pooled.shape)
    else:
        out["y"] = pooled
    out["dp"] = dp
    out["dx"], out["dx_scale"] = tr.pool_dx(dp, g, mode, t["w"], idx)
    if mode == tr.CONV:
        out["dw"], out["dw_scale"] = tr.pool_dw(dp, t["x"], g)
    return out


@pytest.mark.parametrize("c", tr.CASES, ids=tr.case_id)
def test_formulas_equal_the_aten_composition(c):
    g = tr.geo_of(c)
    t = tr.inputs(c, F64, seed=1)
    x, w = t["x"].clone().requires_grad_(), t["w"].to(F64).requires_grad_()
    gamma, beta = t["gamma"].to(F64).requires_grad_(), t["beta"].to(F64).requires_grad_()
    mode = tr.MODES[c["mode"]]
    y = tr.aten_pool(x, g, mode, w, (gamma, beta, tr.EPS) if c["norm"] else None)
    y.backward(t["dy"])
    ref = _ref_chain(c, t, g)
    assert tuple(y.shape) == (g.B, g.rows_out, g.C)
    _close(ref["y"], y.detach(), "y")
    _close(ref["dx"], x.grad, "dx")
    if mode == tr.CONV:
        _close(ref["dw"], w.grad.reshape(g.hd, g.K), "dw")
    if c["norm"]:
        _close(ref["dgamma"], gamma.grad, "dgamma")
        _close(ref["dbeta"], beta.grad, "dbeta")
    if mode == tr.MAX:
        assert tr.window_ties(t["x"], g) == 0
        _, aidx = F.max_pool3d(x.detach()[:, g.cls:].reshape(g.B, *g.thw, g.C).permute(0, 4, 1, 2, 3), g.k, g.s, g.p, return_indices=True)
        cells, _ = g.window()
        mine = torch.gather(cells.t()[None, :, None, :].expand(g.B, g.OL, g.C, g.K), 3, ref["idx"][:, g.cls:].long()[..., None])[..., 0]
        assert torch.equal(mine, aidx.reshape(g.B, g.C, g.OL).transpose(1, 2))


def test_tie_rule_is_atens_first_maximum():
    """All-zero and post-ReLU maps: ATen's CPU kernel keeps the first maximum in (t, h, w) order, and so does pool_fwd."""
    c = tr.CASES[6]
    g = tr.geo_of(c)
    gen = torch.Generator().manual_seed(3)
    for x in (torch.zeros(g.B, g.rows_in, g.C, dtype=F64), torch.randn(g.B, g.rows_in, g.C, generator=gen).clamp_min(0).to(F64)):
        assert tr.window_ties(x, g) > 0
        _, idx, _ = tr.pool_fwd(x, g, tr.MAX)
        _, aidx = F.max_pool3d(x[:, g.cls:].reshape(g.B, *g.thw, g.C).permute(0, 4, 1, 2, 3), g.k, g.s, g.p, return_indices=True)
        cells, _ = g.window()
        mine = torch.gather(cells.t()[None, :, None, :].expand(g.B, g.OL, g.C, g.K), 3, idx[:, g.cls:].long()[..., None])[..., 0]
        assert torch.equal(mine, aidx.reshape(g.B, g.C, g.OL).transpose(1, 2))
        assert not torch.equal(idx, tr.pool_fwd(x, g, tr.MAX, last=True)[1])
        dx, _ = tr.pool_dx(torch.ones(g.B, g.rows_out, g.C, dtype=F64), g, tr.MAX, None, idx)
        xa = x.clone().requires_grad_()
        tr.aten_pool(xa, g, tr.MAX).sum().backward()
        assert torch.equal(dx, xa.grad)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", tr.CASES, ids=tr.case_id)
def test_an_fp32_twin_stays_inside_the_bounds(c, dtype):
    """Every stage in torch float32 (one rounding per operation, the taps in order) from inputs rounded to `dtype`, the result
    rounded to `dtype`: what the kernels compute up to the order of their sums."""
    g = tr.geo_of(c)
    bf = dtype == BF16
    t = tr.inputs(c, dtype, seed=2)
    mode = tr.MODES[c["mode"]]
    ref = _ref_chain(c, t, g)
    tw, tidx, _ = tr.pool_fwd(t["x"], g, mode, t["w"], dtype=F32)
    e, b = tr.pool_fwd_bound(g, ref["scale"], ref["pooled"], bf, mode)
    r = dict(pooled=tr.worst_ratio(tw.to(dtype), ref["pooled"], b))
    if mode == tr.MAX:
        assert torch.equal(tidx, ref["idx"])
    if c["norm"]:
        by, bm, br = tr.norm_fwd_bounds(ref["pooled"], e, g, t["gamma"], t["beta"], tr.EPS, bf)
        p2 = tw.reshape(-1, g.hd)
        mu = p2.mean(-1)
        rs = 1.0 / torch.sqrt(((p2 - mu[:, None]) ** 2).mean(-1) + torch.tensor(tr.EPS, dtype=F32))
        y = ((p2 - mu[:, None]) * rs[:, None] * t["gamma"] + t["beta"]).reshape(tw.shape)
        r.update(y=tr.worst_ratio(y.to(dtype), ref["y"], by), mean=tr.worst_ratio(mu, ref["mean"], bm), rstd=tr.worst_ratio(rs, ref["rstd"], br))
    dp = ref["dp"].to(dtype)                                            # the backward from a stored dpooled
    dx_ref, sc = tr.pool_dx(dp, g, mode, t["w"], ref["idx"])
    dx_tw, _ = tr.pool_dx(dp, g, mode, t["w"], ref["idx"], dtype=F32)
    r["dx"] = tr.worst_ratio(dx_tw.to(dtype), dx_ref, tr.pool_dx_bound(g, sc, dx_ref, bf, mode))
    if mode == tr.CONV:
        dw_ref, sw = tr.pool_dw(dp, t["x"], g)
        dw_tw, _ = tr.pool_dw(dp, t["x"], g, dtype=F32)
        r["dw"] = tr.worst_ratio(dw_tw, dw_ref, tr.pool_dw_bound(g, sw))
    assert all(v <= 1.0 for v in r.values()), r


def test_the_bounds_reject_the_mutants():
    worst = {}
    conv, conv2, avg, mx = tr.CASES[0], tr.CASES[2], tr.CASES[7], tr.CASES[6]
    for dtype in (F32, BF16):
        bf = dtype == BF16
        # conv: the taps in (w, h, t) order; the weight row col / head_dim
        for name, c, kw in (("tap order", conv, dict(tap_perm=[(k % 3) * 9 + ((k // 3) % 3) * 3 + k // 9 for k in range(27)])),
                            ("col / head_dim", conv, dict(wdiv=True)), ("col / head_dim, 3 heads", conv2, dict(wdiv=True))):
            g, t = tr.geo_of(c), tr.inputs(c, dtype, seed=4)
            ref, _, scale = tr.pool_fwd(t["x"], g, tr.CONV, t["w"])
            bad, _, _ = tr.pool_fwd(t["x"], g, tr.CONV, t["w"], **kw)
            worst[name, dtype] = tr.worst_ratio(bad, ref, tr.pool_fwd_bound(g, scale, ref, bf, tr.CONV)[1])
        # avg divided by the in-bounds count
        g, t = tr.geo_of(avg), tr.inputs(avg, dtype, seed=4)
        ref, _, scale = tr.pool_fwd(t["x"], g, tr.AVG)
        bad, _, _ = tr.pool_fwd(t["x"], g, tr.AVG, avg_inbounds=True)
        worst["avg by in-bounds count", dtype] = tr.worst_ratio(bad, ref, tr.pool_fwd_bound(g, scale, ref, bf, tr.AVG)[1])
        # max: the last maximum (post-ReLU map: the index and the gradient move); padding taking part with a 0 (negative map)
        g = tr.geo_of(mx)
        gen = torch.Generator().manual_seed(5)
        x = (torch.randn(g.B, g.rows_in, g.C, generator=gen) - 1).clamp_min(0).to(dtype)      # 84 % zeros: windows tie at 0
        _, idx, _ = tr.pool_fwd(x, g, tr.MAX)
        _, bad_idx, _ = tr.pool_fwd(x, g, tr.MAX, last=True)
        assert not torch.equal(idx, bad_idx)
        dp = torch.randn(g.B, g.rows_out, g.C, generator=gen).to(dtype)
        dx, sc = tr.pool_dx(dp, g, tr.MAX, None, idx)
        bad, _ = tr.pool_dx(dp, g, tr.MAX, None, bad_idx)
        worst["last maximum", dtype] = tr.worst_ratio(bad, dx, tr.pool_dx_bound(g, sc, dx, bf, tr.MAX))
        neg = (-torch.rand(g.B, g.rows_in, g.C, generator=gen) - 1.0).to(dtype)
        ref, _, scale = tr.pool_fwd(neg, g, tr.MAX)
        bad, _, _ = tr.pool_fwd(neg, g, tr.MAX, admit_pad=True)
        worst["padding as 0 in max", dtype] = tr.worst_ratio(bad, ref, tr.pool_fwd_bound(g, scale, ref, bf, tr.MAX)[1])
        # the cls row normalised with the statistics of the next head
        g, t = tr.geo_of(conv), tr.inputs(conv, dtype, seed=4)
        pooled, _, scale = tr.pool_fwd(t["x"], g, tr.CONV, t["w"])
        e, _ = tr.pool_fwd_bound(g, scale, pooled, bf, tr.CONV)
        y, mean, rstd = tr.norm_fwd(pooled, g, t["gamma"], t["beta"], tr.EPS)
        by, _, _ = tr.norm_fwd_bounds(pooled, e, g, t["gamma"], t["beta"], tr.EPS, bf)
        m2, r2 = mean.view(g.B, g.rows_out, g.heads).roll(1, 2), rstd.view(g.B, g.rows_out, g.heads).roll(1, 2)
        p4 = pooled.view(g.B, g.rows_out, g.heads, g.hd)
        bad = y.clone().view(g.B, g.rows_out, g.heads, g.hd)
        bad[:, 0] = (p4[:, 0] - m2[:, 0, :, None]) * r2[:, 0, :, None] * t["gamma"].to(F64) + t["beta"].to(F64)
        worst["cls row, another head's statistics", dtype] = tr.worst_ratio(bad.view_as(y), y, by)
    assert all(v > 1.0 for v in worst.values()), worst


# ---- the host side of the library ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import focus_amd.build as fb
    fb.build(verbose=False)
    from focus_amd import _lib
    return _lib.lib()


def _desc(g, mode, dtype=F32, xrs=1):
    from focus_amd import _lib
    d = _lib.TokenPoolDesc()
    d.B, d.T, d.H, d.W, d.C, d.head_dim, d.cls = g.B, g.thw[0], g.thw[1], g.thw[2], g.C, g.hd, g.cls
    for i in range(3):
        d.k[i], d.s[i], d.p[i] = g.k[i], g.s[i], g.p[i]
    d.mode, d.dtype = mode, _lib.BF16 if dtype == BF16 else _lib.F32
    d.x_row_stride, d.x_batch_stride = xrs * g.C, g.rows_in * xrs * g.C
    return d


def test_descriptor_layout_matches_the_header():
    from focus_amd import _lib
    src = open(_lib.HEADER).read()
    body = re.search(r"typedef struct focus_token_pool_desc \{(.*?)\} focus_token_pool_desc;", src, re.S).group(1)
    fields, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        size = {"int32_t": 4, "int64_t": 8}[ty]
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            off = (off + size - 1) // size * size
            fields.append((m.group(1), off, size * int(m.group(2) or 1)))
            off += size * int(m.group(2) or 1)
    D = _lib.TokenPoolDesc
    assert [(n, getattr(D, n).offset, getattr(D, n).size) for n, _ in D._fields_] == fields
    assert ctypes.sizeof(D) == (off + 7) // 8 * 8 == 88
    assert (_lib.POOL_CONV, _lib.POOL_MAX, _lib.POOL_AVG) == (tr.CONV, tr.MAX, tr.AVG)
    assert re.search(r"FOCUS_POOL_CONV = 0, FOCUS_POOL_MAX = 1, FOCUS_POOL_AVG = 2", src)


def test_grid_walk_matches_the_library(lib):
    cases = tr.CASES + [tr.big_case(lambda g, stage: tr.blocks(g, stage))]
    for c in cases:
        g = tr.geo_of(c)
        d = _desc(g, tr.MODES[c["mode"]])
        for stage in range(4):
            if stage == 1 and g.hd > 128:
                assert lib.focus_token_pool_blocks(ctypes.byref(d), stage) == 0
                continue
            assert lib.focus_token_pool_blocks(ctypes.byref(d), stage) == tr.blocks(g, stage), (tr.case_id(c), stage)
        assert lib.focus_token_pool_workspace_bytes(ctypes.byref(d)) == (tr.workspace_bytes(g) if c["mode"] == "conv" else 0)
    big = tr.geo_of(cases[-1])
    assert tr.fwd_lanes(big, True) > tr.MAX_BLOCKS * tr.THREADS and tr.dw_blocks(big) > 64
    assert tr.dw_tiles(tr.geo_of(tr.CASES[11])) == 2 and tr.geo_of(tr.CASES[10]).hd * tr.geo_of(tr.CASES[10]).K > tr.WLDS_FLOATS
    assert lib.focus_token_pool_blocks(None, 0) == 0 and lib.focus_token_pool_blocks(ctypes.byref(d), 4) == 0


def test_every_status_before_a_launch_in_the_documented_order(lib):
    """No GPU here: a call that got past its checks would fail to launch (FOCUS_ERR_LAUNCH), so every code below is the
    entry point's own verdict.  Order: NULL (d), SHAPE, DTYPE, OK for B == 0, NULL (buffers), ALIGN, WORKSPACE."""
    OK, SHAPE, DTYPE, ALIGN, NULL, WORKSPACE = 0, -1, -2, -3, -5, -6
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr, odd = ctypes.c_void_p(a), ctypes.c_void_p(a + 8)
    g = tr.geo_of(tr.CASES[0])

    def fwd(d, x=ptr, w=ptr, gamma=ptr, beta=ptr, y=ptr, pooled=ptr, mean=ptr, rstd=ptr, idx=None):
        return lib.focus_token_pool_fwd(ctypes.byref(d) if d is not None else None, x, w, gamma, beta, 1e-6, y, pooled, mean, rstd, idx, None)

    def bwd(d, dp=ptr, x=ptr, w=ptr, idx=None, dx=ptr, dw=ptr, ws=ptr, nbytes=1 << 30):
        return lib.focus_token_pool_bwd(ctypes.byref(d) if d is not None else None, dp, x, w, idx, dx, dw, ws, nbytes, None)

    assert fwd(None) == NULL and bwd(None) == NULL
    def bad(**kw):
        d = _desc(g, tr.CONV)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d
    shape = [dict(B=-1), dict(T=0), dict(H=0), dict(W=0), dict(C=36), dict(C=4104, head_dim=8), dict(head_dim=12), dict(head_dim=24),
             dict(C=256, head_dim=256), dict(cls=2), dict(mode=3), dict(mode=-1), dict(k=(0, 0)), dict(k=(1, 8)), dict(s=(2, 0)), dict(s=(2, 9)),
             dict(p=(1, 3)), dict(p=(1, -1)), dict(T=1, k=(0, 5), p=(0, 1)), dict(x_row_stride=24), dict(x_batch_stride=-32),
             dict(B=1 << 20, T=64, H=64, W=64)]
    for kw in shape:
        # SHAPE before everything but a NULL descriptor: the pointers are NULL, the dtype unknown, the strides misaligned
        d = bad(dtype=7, **kw)
        if "x_row_stride" not in kw:
            d.x_row_stride = g.C + 1
        assert lib.focus_token_pool_fwd(ctypes.byref(d), None, None, ptr, ptr, 1e-6, None, None, None, None, None, None) == SHAPE, kw
        assert lib.focus_token_pool_bwd(ctypes.byref(d), None, None, None, None, None, None, None, 0, None) == SHAPE, kw
        assert lib.focus_token_pool_blocks(ctypes.byref(d), 0) == 0 and lib.focus_token_pool_workspace_bytes(ctypes.byref(d)) == 0
    d = bad(mode=tr.MAX, k=(0, 7), p=(0, 3))
    d.k[1], d.k[2], d.p[1], d.p[2] = 7, 7, 3, 3
    d.T = d.H = d.W = 8
    assert fwd(d) == SHAPE                                              # 343 taps do not fit the int8 index
    d = bad(C=256, head_dim=256, mode=tr.MAX)
    assert fwd(d, idx=ptr) == SHAPE                                     # the norm needs head_dim <= 128
    assert bwd(bad(mode=tr.MAX), idx=ptr) == SHAPE                      # dw outside conv mode
    # DTYPE next: pointers NULL and strides misaligned still
    d = bad(dtype=2, x_row_stride=g.C + 1)
    assert lib.focus_token_pool_fwd(ctypes.byref(d), None, None, None, None, 1e-6, None, None, None, None, None, None) == DTYPE
    assert lib.focus_token_pool_bwd(ctypes.byref(d), None, None, None, None, None, None, None, 0, None) == DTYPE
    # B == 0: nothing to do, whatever the pointers hold
    assert lib.focus_token_pool_fwd(ctypes.byref(bad(B=0)), None, None, None, None, 1e-6, None, None, None, None, None, None) == OK
    assert lib.focus_token_pool_bwd(ctypes.byref(bad(B=0)), None, None, None, None, None, None, None, 0, None) == OK
    # NULL buffers before ALIGN: the other pointers are misaligned
    d = bad()
    for kw in (dict(x=None), dict(y=None), dict(w=None), dict(gamma=None), dict(beta=None), dict(pooled=None), dict(mean=None), dict(rstd=None)):
        args = dict(x=odd, w=odd, y=odd)
        args.update(kw)
        assert fwd(d, **args) == NULL, kw
    assert fwd(bad(mode=tr.MAX), x=odd, idx=None) == NULL
    for kw in (dict(dp=None), dict(dx=None, dw=None), dict(w=None), dict(x=None), dict(ws=None)):
        args = dict(dp=odd)
        args.update(kw)
        assert bwd(d, **args) == NULL, kw
    assert bwd(bad(mode=tr.MAX), dw=None, idx=None, dp=odd) == NULL
    # ALIGN before WORKSPACE
    for kw in (dict(x=odd), dict(w=odd), dict(gamma=odd), dict(beta=odd), dict(y=odd), dict(pooled=odd), dict(mean=odd), dict(rstd=odd)):
        assert fwd(d, **kw) == ALIGN, kw
    assert fwd(bad(mode=tr.MAX), idx=odd) == ALIGN
    assert fwd(bad(x_row_stride=g.C + 1)) == ALIGN and fwd(bad(x_batch_stride=g.rows_in * g.C + 2)) == ALIGN
    assert fwd(bad(dtype=1, x_row_stride=g.C + 4)) == ALIGN             # bf16: 8 elements
    for kw in (dict(dp=odd), dict(x=odd), dict(w=odd), dict(dx=odd), dict(dw=odd), dict(ws=odd)):
        assert bwd(d, nbytes=0, **kw) == ALIGN, kw
    need = lib.focus_token_pool_workspace_bytes(ctypes.byref(d))
    assert need == tr.workspace_bytes(g) > 0
    assert bwd(d, nbytes=need - 1) == WORKSPACE and bwd(d, nbytes=0) == WORKSPACE


def test_token_pool_ok_truth_table():
    from focus_amd import ops
    x = torch.zeros(2, 1 + 2 * 5 * 7, 32)
    norm = nn.LayerNorm(16)
    w = torch.zeros(16, 1, 3, 3, 3)
    base = (x, 16, "conv", (3, 3, 3), (1, 2, 2), (1, 1, 1), norm, w)
    assert not ops.token_pool_ok(*base)                                 # a CPU tensor: the ATen path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_pool(x, (2, 5, 7), "conv", w, (3, 3, 3), (1, 2, 2), (1, 1, 1), True, 16, norm)
    ok = ops._token_pool_limits_ok
    assert ok(*base) and ok(x.bfloat16(), *base[1:]) and ok(x, 16, "conv", 3, [1, 2, 2], 1, (norm.weight, norm.bias, 1e-6), w)
    wide = torch.zeros(2, 71, 96)
    assert ok(wide[:, :, 32:64], *base[1:]) and not ok(wide[:, :, 2:34], *base[1:]) and not ok(wide.transpose(1, 2)[:, :32, :71], 16, "max", 1, 1, 0, None)
    assert ok(torch.zeros(2, 9, 768), 768, "max", (1, 3, 3), (1, 2, 2), (0, 1, 1), None)          # the skip pool: head_dim = C
    assert ok(torch.zeros(2, 9, 768), 96, "conv", 3, 1, 1, nn.LayerNorm(96), torch.zeros(96, 1, 3, 3, 3))
    refused = [
        (x.double(),) + base[1:], (x[0],) + base[1:], (x, 12) + base[2:], (x, 24) + base[2:], (x, 16, "sum") + base[3:],
        (x, 16, "conv", (3, 3)) + base[4:], (x, 16, "conv", (8, 3, 3)) + base[4:], (x, 16, "conv", (3, 3, 3), (1, 9, 9)) + base[5:],
        (x, 16, "conv", (3, 3, 3), (1, 0, 2)) + base[5:], (x, 16, "conv", (3, 3, 3), (1, 2, 2), (1, 1, 3)) + base[6:],
        (x, 16, "conv", (3, 3, 3), (1, 2, 2), (1, 1, -1)) + base[6:],
        (torch.zeros(2, 9, 256), 256, "conv", 3, 1, 1, None, torch.zeros(256, 1, 3, 3, 3)),           # head_dim > 128 in conv mode
        (torch.zeros(2, 9, 256), 256, "max", 3, 1, 1, nn.LayerNorm(256)),                               # ... or with a norm
        (torch.zeros(1, 9, 4104), 8, "max", 3, 1, 1, None),                                             # C > 4096
        (x, 16, "max", (7, 7, 7), 1, 3, None),                                                          # 343 taps
        base[:6] + (nn.LayerNorm(16).double(), w), base[:7] + (w.double(),), base[:7] + (torch.zeros(16, 1, 3, 3, 1),),
        base[:6] + (nn.LayerNorm(32), w),
    ]
    for i, args in enumerate(refused):
        assert not ok(*args), i


def test_cpu_tensors_keep_the_aten_path(monkeypatch):
    """The MViT modules built and called on the CPU: ops.token_pool is never reached (it raises on CPU tensors), the pooling
    runs through attention_pool as before, and the state-dict keys are what they were."""
    from focus_amd import ops
    from focus_amd.slowfast.models import attention as A

    def never(*a, **k):
        raise AssertionError("ops.token_pool reached with CPU tensors")
    monkeypatch.setattr(ops, "token_pool", never)
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None, residual=None, alpha=1.0: F.linear(x, w, b) if residual is None else F.linear(x, w, b) + residual)
    monkeypatch.setattr(ops, "layer_norm", lambda x, g, b, eps: F.layer_norm(x, (x.shape[-1],), g, b, eps))
    monkeypatch.setattr(ops, "flash_ok", lambda *a: False)

    def attn(q, k, v, heads, scale, causal=False, drop=None):
        B, n, C = q.shape
        h = lambda t: t.reshape(B, -1, heads, C // heads).transpose(1, 2)
        return (torch.softmax(h(q) * scale @ h(k).transpose(-1, -2), -1) @ h(v)).transpose(1, 2).reshape(B, n, C)
    monkeypatch.setattr(ops, "small_attention", attn)
    torch.manual_seed(0)
    thw = [2, 4, 4]
    x = torch.randn(2, 33, 32)
    for pool_first in (False, True):
        m = A.MultiScaleAttention(32, num_heads=2, kernel_q=(3, 3, 3), kernel_kv=(3, 3, 3), stride_q=(1, 2, 2), stride_kv=(1, 2, 2),
                                  pool_first=pool_first)
        assert sorted(m.state_dict()) == sorted(["q.weight", "k.weight", "v.weight", "proj.weight", "proj.bias", "pool_q.weight", "norm_q.weight",
                                                 "norm_q.bias", "pool_k.weight", "norm_k.weight", "norm_k.bias", "pool_v.weight",
                                                 "norm_v.weight", "norm_v.bias"])
        y, shape = m(x, thw)
        assert tuple(y.shape) == (2, 9, 32) and shape == [2, 2, 2]
        # the rows route equals attention_pool on the head-split tensor, bit for bit
        q = F.linear(x, m.q.weight) if not pool_first else x
        a, _ = A.pool_rows(q, m.pool_q, thw, True, m.norm_q, 2)
        b, _ = A.attention_pool(q.reshape(2, 33, 2, 16).permute(0, 2, 1, 3), m.pool_q, thw, True, m.norm_q)
        assert torch.equal(a, b.permute(0, 2, 1, 3).reshape(2, 9, 32))
    skip = nn.MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1))
    a, shape = A.pool_rows(x, skip, thw, True, None, 1)
    b, _ = A.attention_pool(x, skip, thw, True)
    assert torch.equal(a, b) and shape == [2, 2, 2]
    assert A._pool_spec(nn.Conv3d(16, 16, 3, groups=16, bias=True)) is None and A._pool_spec(nn.Conv3d(16, 16, 3, bias=False)) is None
    assert A._pool_spec(nn.MaxPool3d(3, 2, 1, ceil_mode=True)) is None and A._pool_spec(nn.AvgPool3d(3, 2, 1, count_include_pad=False)) is None
    assert A._pool_spec(nn.AvgPool3d(3, 2, 1))[0] == "avg" and A._pool_spec(nn.Identity()) is None
