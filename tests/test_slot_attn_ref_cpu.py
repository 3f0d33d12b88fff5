"""tests/slot_attn_ref.py checked without a GPU: the closed-form backward equals torch.autograd in fp64 on every case of the
table (with and without a cotangent of attn_vis, with both eps), and every case reaches the kernel its label names, by
focus_slot_attn_route -- the host function the entry points take their dispatch from."""
import os

import pytest
import torch

import slot_attn_ref as sa

IDS = [c.name for c in sa.CASES]
SWITCHES = ("FOCUS_SLOT_MFMA", "FOCUS_SLOT_KV_DEFER")       # read once per process: with one set the route is reported


@pytest.fixture(scope="module")
def lib():
    from focus_amd.build import build
    build(verbose=False)
    from focus_amd import _lib
    return _lib.lib()


def _close(got, want, what):
    err, top = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
    assert err <= 1e-10 * top, (what, err, top)


@pytest.mark.parametrize("case", sa.CASES, ids=IDS)
def test_closed_form_backward_is_autograd(case):
    x = sa.inputs(case)
    for dupd, dattn in ((x["dupd1"], x["dattn1"]), (x["dupd2"], None)):
        k, v, q = (x[n].double().requires_grad_() for n in ("k", "v", "q"))
        attn, colsum, upd = sa.forward(k, v, q, case.eps)
        loss = (upd * dupd.double()).sum()
        if dattn is not None:
            loss = loss + (attn * dattn.double()).sum()
        loss.backward()
        with torch.no_grad():
            r = sa.backward(k, v, q, attn, colsum, upd, dupd, dattn, case.eps)
        _close(r["dk"], k.grad, "dk")
        _close(r["dv"], v.grad, "dv")
        _close(r["dq"], q.grad, "dq")
        assert bool((r["w"].sum(1) - 1).abs().max() < 1e-12)                 # the weights of a mean
        if case.K == 1:
            assert bool((attn == 1).all()) and bool((r["dlogits"] == 0).all())


def test_kv_grad_is_the_sum_over_the_iterations():
    case = sa.CASES[0]
    x = sa.inputs(case)
    attn, colsum, upd = sa.forward(x["k"], x["v"], x["q"], case.eps)
    rs = [sa.backward(x["k"], x["v"], x["q"], attn, colsum, upd, x[d], None, case.eps) for d in ("dupd1", "dupd2")]
    wls = []
    for r in rs:
        wl = torch.zeros(case.B, case.N, 32, dtype=torch.float64)
        wl[..., :case.K], wl[..., 16:16 + case.K] = r["w"], r["dlogits"]
        wls.append(wl)
    dk, dv, _, _ = sa.kv_grad(wls, [x["q"]] * 2, [x["dupd1"], x["dupd2"]])
    _close(dk, rs[0]["dk"] + rs[1]["dk"], "dk")
    _close(dv, rs[0]["dv"] + rs[1]["dv"], "dv")


def test_the_table_holds_what_it_promises():
    cs = sa.CASES
    assert len({c.name for c in cs}) == len(cs)
    assert all(c.B <= 3 and c.N <= 1100 and c.eps in (sa.EPS_SMALL, sa.EPS_BIG) for c in cs)
    assert sum(c.big for c in cs) * 3 >= len(cs)
    gen32 = [c for c in cs if c.dtype == "f32"]
    assert {(c.fwd[2], c.fwd[3]) for c in gen32} >= {(4, 1), (8, 2), (16, 3), (16, 4), (32, 1), (32, 4)}
    assert sum(c.eps == sa.EPS_BIG for c in gen32) == 2
    assert {c.N for c in cs if c.wl and (c.K, c.D) == (11, 192)} >= {1, 15, 16, 17, 33, 255, 256, 257, 700}
    assert {(c.N, c.K, c.D) for c in cs if c.bwd[0] == sa.BWD_MFMA} >= {
        (N, K, D) for N in (256, 257, 33) for K in (3, 16) for D in (64, 128, 192, 256)}
    for c in cs:                                                             # logits of the scaled cases span about +-20
        if c.big and c.N * c.K >= 256:
            x = sa.inputs(c)
            lg = x["k"].double() @ x["q"].double().transpose(-1, -2)
            assert 12 < float(lg.max()) and float(lg.min()) < -12, (c.name, float(lg.min()), float(lg.max()))


def fake_pointers(case):
    """Addresses with the alignment the GPU test's buffers have (the route only looks at the low bits)."""
    esize = 2 if case.dtype == "bf16" else 4
    base = 1 << 20
    return {"k": base + case.k_off * esize, "v": 2 * base, "q": 3 * base, "dk": 4 * base, "dv": 5 * base, "wl": 6 * base}


def routes(L, case, p):
    from focus_amd import _lib
    dt = _lib.BF16 if case.dtype == "bf16" else _lib.F32
    kv_bs = case.N * case.D + case.kv_gap
    fwd = L.focus_slot_attn_route(0, p["k"], p["v"], kv_bs, p["q"], None, None, None, case.N, case.K, case.D, dt)
    bwd = L.focus_slot_attn_route(1, p["k"], p["v"], kv_bs, p["q"], None if case.wl else p["dk"], None if case.wl else p["dv"],
                                  p["wl"] if case.wl else None, case.N, case.K, case.D, dt)
    return sa.decode_route(fwd), sa.decode_route(bwd)


@pytest.mark.parametrize("case", sa.CASES, ids=IDS)
def test_every_case_reaches_the_route_it_names(case, lib, monkeypatch):
    if case.hand is not None:
        monkeypatch.setenv("FOCUS_SLOT_HAND", case.hand)
    else:
        monkeypatch.delenv("FOCUS_SLOT_HAND", raising=False)
    fwd, bwd = routes(lib, case, fake_pointers(case))
    print(case.name, fwd, bwd)
    if any(os.environ.get(s) for s in SWITCHES):
        return
    assert fwd == case.fwd and bwd == case.bwd, (case.name, fwd, case.fwd, bwd, case.bwd)


def test_route_refuses_what_the_entry_points_refuse(lib):
    from focus_amd import _lib
    p = 1 << 20
    SHAPE, ALIGN = -1, lib.focus_slot_attn_route(1, p + 2, p, 256 * 64, p, None, None, p, 256, 4, 64, _lib.BF16)
    assert lib.focus_strerror(SHAPE) == b"bad shape" and ALIGN < 0 and ALIGN != SHAPE
    assert lib.focus_slot_attn_route(0, p, p, 256 * 64, p, None, None, None, 256, 33, 64, _lib.BF16) == SHAPE
    assert lib.focus_slot_attn_route(0, p, p, 256 * 300, p, None, None, None, 256, 4, 300, _lib.F32) == SHAPE
    assert lib.focus_slot_attn_route(1, p, p, 256 * 64, p, None, None, p, 256, 4, 64, _lib.F32) == SHAPE   # wl is bf16 only
    # a dk_t that is not 8-byte aligned sends the non-deferred backward to the generic kernel
    r = sa.decode_route(lib.focus_slot_attn_route(1, p, p, 256 * 64, p, p + 2, p, None, 256, 4, 64, _lib.BF16))
    assert r == (sa.BWD_GENERIC, 0, 4, 1)
