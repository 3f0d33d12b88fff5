"""tests/ln_ref.py checked without a GPU: the fp64 reference against torch's LayerNorm through autograd, an fp32 twin of each
kernel family inside the derived bounds on every case of the table (a bound that is too tight shows here, not on the GPU
machine), every mutant outside them, the routes the table reaches, and the argument checks of the four LayerNorm entry
points of csrc/layernorm.hip (refusals only: a valid call would launch).

The twins are torch float32 on the CPU: one IEEE rounding per operation, the order of operations of the kernels."""
import ctypes

import pytest
import torch

import ln_ref as lr

F64 = torch.float64


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_reference_is_torch_layer_norm_in_fp64():
    g = torch.Generator().manual_seed(5)
    for rows, D, eps in ((9, 12, 1e-6), (33, 260, 1e-5), (5, 1028, 1e-6)):
        x = (torch.randn(rows, D, generator=g, dtype=F64) * 2 + 0.5).requires_grad_()
        gamma, beta = (torch.randn(D, generator=g, dtype=F64).requires_grad_() for _ in range(2))
        cy, dres = torch.randn(rows, D, generator=g, dtype=F64), torch.randn(rows, D, generator=g, dtype=F64)
        y = torch.nn.functional.layer_norm(x, (D,), gamma, beta, eps)
        ((y * cy).sum() + (x * dres).sum()).backward()                 # the residual path hands dres to x unchanged
        ry, mean, rstd = lr.fwd(x.detach(), gamma.detach(), beta.detach(), eps)
        assert _rel(ry, y.detach()) <= 1e-12
        assert _rel(mean, x.detach().mean(-1)) <= 1e-12
        assert _rel(rstd, 1 / torch.sqrt(x.detach().var(-1, unbiased=False) + eps)) <= 1e-12
        dx, dg, db = lr.bwd(cy, x.detach(), gamma.detach(), mean, rstd, dres)
        assert _rel(dx, x.grad) <= 1e-12 and _rel(dg, gamma.grad) <= 1e-12 and _rel(db, beta.grad) <= 1e-12
        dx0 = lr.bwd(cy, x.detach(), gamma.detach(), mean, rstd)[0]
        assert _rel(dx0 + dres, x.grad) <= 1e-12


def test_block_addressing_is_slicing_a_video():
    B, T, N, D = 3, 3, 7, 12
    video = torch.arange(B * T * N * D, dtype=F64).view(B, T, N, D)
    for t in range(T):
        got = lr.gather_rows(video.view(-1), t * N * D, B * N, N, T * N * D, D)
        assert torch.equal(got, video[:, t].reshape(B * N, D))
        out = torch.zeros(B * T * N * D, dtype=F64)
        lr.scatter_rows(out, t * N * D, got, N, T * N * D)
        want = torch.zeros(B, T, N, D, dtype=F64)
        want[:, t] = video[:, t]
        assert torch.equal(out.view(B, T, N, D), want)
    assert torch.equal(lr.row_offsets(5, 5, 0, 4), torch.arange(5) * 4)          # dense: rpb = rows, xbs = 0


CPU_GROUPS = [g for g in lr.GROUPS if all(c["rows"] <= 2 ** 16 for c in lr.group(g))]


@pytest.mark.parametrize("name", CPU_GROUPS)
def test_fp32_twin_stays_inside_the_bounds(name):
    for c in lr.group(name):
        t = lr.inputs(c)
        r = lr.route_of(c)
        if c["dir"] == "fwd":
            y, mean, rstd = lr.twin_fwd(t["x"], t["gamma"], t["beta"], t["eps"], r)
            ratios = lr.fwd_ratios(c, t, dict(y=y, mean=mean, rstd=rstd))
        else:
            mean, rstd = lr.ref_stats(t, c["rows"])
            dx, dg, db, partial = lr.twin_bwd(t["dy"], t["x"], t["gamma"], mean, rstd, t["dres"], r)
            ratios = lr.bwd_ratios(c, t, mean, rstd, dict(dx=dx, dgamma=dg, dbeta=db, partial=partial))
        print("%-48s %s" % (lr.case_id(c), "  ".join("%s %.3f" % kv for kv in ratios.items())))
        assert all(v <= 1.0 for v in ratios.values()), (lr.case_id(c), ratios)


def test_every_mutant_exceeds_a_bound():
    for name, mutant, applies in lr.MUTANTS:
        cases = [c for c in lr.CASES if applies(c)]
        assert cases, name
        worst = 0.0
        for c in cases:
            t = lr.inputs(c)
            got = mutant(c, t)
            if c["dir"] == "fwd":
                ratios = lr.fwd_ratios(c, t, got)
            else:
                mean, rstd = lr.ref_stats(t, c["rows"])
                ratios = lr.bwd_ratios(c, t, mean, rstd, got)
            worst = max(worst, max(ratios.values()))
        print("%-48s over %3d cases: largest error / bound %.3g" % (name, len(cases), worst))
        assert worst > 1.0, name


def test_the_table_reaches_every_route():
    got = set()
    for c in lr.CASES:
        r = lr.route_of(c)
        blocks = c["rpb"] is not None
        if r["family"] == "wave":
            got.add(("wave", c["dir"], c["dtype"], r["NV"]))
            if blocks:
                got.add(("wave", c["dir"], "blocks"))
            if c["dir"] == "bwd" and r["trips"] > 1:
                got.add(("wave", "bwd", "row loop twice"))
        elif c["dir"] == "fwd":
            got.add(("sub", "fwd", r["LPR"], r["NV"], "two trips" if r["trips"] > 1 else "one trip"))
            if blocks:
                got.add(("sub", "fwd", "blocks"))
        else:
            got.add(("sub", "bwd", r["LPR"], r["NV"], r["NW"], "dres" if c["dres"] else "no dres"))
            if blocks:
                got.add(("sub", "bwd", "blocks"))
            if r["NW"] == 8 and c["D"] == 1024:
                assert r["lds"] == 65536
    want = {("wave", d, t, nv) for d in ("fwd", "bwd") for t in ("fp32", "bf16") for nv in (1, 2, 3, 4, 8, 16)}
    want |= {(f, d, "blocks") for f in ("wave", "sub") for d in ("fwd", "bwd")}
    want.add(("wave", "bwd", "row loop twice"))
    pairs = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2))
    want |= {("sub", "fwd", l, n, trips) for l, n in pairs for trips in ("one trip", "two trips")}
    want |= {("sub", "bwd", l, n, nw, dres) for l, n in pairs for nw in (4, 8) for dres in ("dres", "no dres")}
    assert got == want, (sorted(map(str, want - got)), sorted(map(str, got - want)))
    # the bf16 cases of >= 4096 rows that have to stay wave per row do
    for c in lr.group("wave-fwd-bf16-4100") + lr.group("wave-bwd-bf16-4100"):
        assert lr.route_of(c)["family"] == "wave" and c["rows"] >= 4096
    # and the blocks of the library agree with the twin
    assert [lr.bwd_blocks(r) for r in (0, 1, 4, 5, 2047, 2048, 2049, 10 ** 6)] == [1, 1, 1, 2, 512, 512, 512, 512]


def test_layernorm_entry_points_validate_before_launching(built):
    """Refusals only, with the status the header states; no call here reaches a launch."""
    from focus_amd import _lib
    lib = _lib.lib()
    F32, BF16 = _lib.F32, _lib.BF16
    OK, SHAPE, ALIGN, NULL = 0, -1, -3, -5
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    a += -a % 16
    p, p4, p8 = ctypes.c_void_p(a), ctypes.c_void_p(a + 4), ctypes.c_void_p(a + 8)
    rows, D = 5, 8
    assert [lib.focus_layernorm_bwd_blocks(r) for r in (0, 1, 5, 2049)] == [lr.bwd_blocks(r) for r in (0, 1, 5, 2049)]

    def fwd(x=p, g=p, b=p, y=p, m=p, r=p, rows=rows, D=D, dt=F32):
        return lib.focus_layernorm_fwd(x, g, b, y, m, r, rows, D, 1e-6, dt, None)

    def fwdb(x=p, rpb=rows, xbs=0, g=p, b=p, y=p, m=p, r=p, rows=rows, D=D, dt=F32):
        return lib.focus_layernorm_fwd_blocks(x, rpb, xbs, g, b, y, m, r, rows, D, 1e-6, dt, None)

    def bwd(dy=p, x=p, g=p, m=p, r=p, dres=None, dx=p, dg=p, db=p, part=p, rows=rows, D=D, dt=F32):
        return lib.focus_layernorm_bwd(dy, x, g, m, r, dres, dx, dg, db, part, rows, D, dt, None)

    def bwdb(dy=p, x=p, rpb=rows, xbs=0, g=p, m=p, r=p, dx=p, dg=p, db=p, part=p, rows=rows, D=D, dt=F32):
        return lib.focus_layernorm_bwd_blocks_strided(dy, x, rpb, xbs, g, m, r, dx, dg, db, part, rows, D, dt, None)

    for k in ("x", "g", "b", "y", "m", "r"):
        assert fwd(**{k: None}) == NULL and fwdb(**{k: None}) == NULL, k
    for k in ("dy", "x", "g", "m", "r", "dx", "part"):
        assert bwd(**{k: None}) == NULL and bwdb(**{k: None}) == NULL, k
    for call in (bwd, bwdb):
        assert call(dg=None) == NULL and call(db=None) == NULL           # dgamma without dbeta, and the reverse
    for call in (fwd, fwdb, bwd, bwdb):
        for bad in (0, 6, 4100, -4):
            assert call(D=bad) == SHAPE, (call.__name__, bad)
    for call in (fwdb, bwdb):
        assert call(rpb=0) == SHAPE and call(rpb=-1) == SHAPE
        assert call(xbs=6) == SHAPE and call(xbs=4 * D + 2) == SHAPE
    assert bwd(rows=-1) == SHAPE and bwdb(rows=-1) == SHAPE
    # alignment: 4 elements of the type for the row pointers (16 bytes fp32, 8 bytes bf16), 16 bytes for gamma and beta
    for call in (fwd, fwdb):
        for k in ("x", "y"):
            assert call(**{k: p8}) == ALIGN and call(**{k: p4}) == ALIGN, k
            assert call(**{k: p4, "dt": BF16}) == ALIGN, k
        assert call(g=p8) == ALIGN and call(b=p8) == ALIGN and call(g=p8, dt=BF16) == ALIGN
    for call in (bwd, bwdb):
        for k in ("dy", "x", "dx"):
            assert call(**{k: p8}) == ALIGN and call(**{k: p4}) == ALIGN, k
            assert call(**{k: p4, "dt": BF16}) == ALIGN, k
        assert call(g=p8) == ALIGN and call(g=p8, dt=BF16) == ALIGN
    assert bwd(dres=p8) == ALIGN and bwd(dres=p4, dt=BF16) == ALIGN
    # shape is judged before alignment, NULL before both; no rows: the forward has nothing to do
    assert fwd(x=p4, D=6) == SHAPE and bwd(x=p4, D=6) == SHAPE and bwd(x=None, D=6) == NULL
    assert fwd(rows=0) == OK and fwdb(rows=0) == OK and fwd(rows=0, x=None, y=None, m=None, r=None) == OK
    assert fwd(rows=0, g=None) == NULL and bwd(rows=0, part=None) == NULL and bwd(rows=0, dg=None) == NULL
    assert bwd(rows=0, D=6) == SHAPE and bwd(rows=0, x=p4) == ALIGN
