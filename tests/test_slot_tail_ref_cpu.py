"""tests/slot_tail_ref.py is the yardstick of tests/test_gpu_slot_tail.py; this pins it without a GPU: the chained form
against torch.nn's own GRUCell / LayerNorm / Linear in fp64 (values and autograd gradients), the stage functions of the
backward against autograd on the chained form, the per-block LayerNorm partials against the LayerNorm parameter gradients,
and the conditions that make the seeded inputs of the GPU test a test (ReLU both ways, gates not saturated, no flat row)."""
import pytest
import torch

import slot_tail_ref as sr

D, H = sr.D, sr.H
TOL = 1e-10


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _modules(p):
    f64 = lambda t: torch.nn.Parameter(t.double().clone())
    gru = torch.nn.GRUCell(D, D).double()
    gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh = f64(p["w_ih"]), f64(p["w_hh"]), f64(p["b_ih"]), f64(p["b_hh"])
    ln1, ln2 = torch.nn.LayerNorm(D, eps=sr.EPS).double(), torch.nn.LayerNorm(D, eps=sr.EPS).double()
    ln1.weight, ln1.bias, ln2.weight, ln2.bias = f64(p["ln1_g"]), f64(p["ln1_b"]), f64(p["ln2_g"]), f64(p["ln2_b"])
    mlp = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(), torch.nn.Linear(H, D)).double()
    mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias = f64(p["w1"]), f64(p["b1"]), f64(p["w2"]), f64(p["b2"])
    wq = torch.nn.Linear(D, D, bias=False).double()
    wq.weight = f64(p["wq"])
    named = {"w_ih": gru.weight_ih, "w_hh": gru.weight_hh, "b_ih": gru.bias_ih, "b_hh": gru.bias_hh, "ln1_g": ln1.weight,
             "ln1_b": ln1.bias, "w1": mlp[0].weight, "b1": mlp[0].bias, "w2": mlp[2].weight, "b2": mlp[2].bias,
             "ln2_g": ln2.weight, "ln2_b": ln2.bias, "wq": wq.weight}
    return gru, ln1, mlp, ln2, wq, named


@pytest.mark.parametrize("name", list(sr.FLAGS))
def test_chained_form_is_torch_nn_in_fp64(name):
    """Outputs and autograd gradients of both inputs and all thirteen parameters, per flag combination (a parameter of a
    stage that is switched off has no gradient on either side)."""
    gru_f, mlp_f, q_f = sr.FLAGS[name]
    R = 17
    p = sr.make_params()
    upd0, h0 = sr.make_rows(R)
    cs, cq = (t.double() for t in sr.make_grads(R))
    gru, ln1, mlp, ln2, wq, named = _modules(p)
    upd, h = upd0.double().requires_grad_(), h0.double().requires_grad_()
    cur = h
    if gru_f:
        cur = gru(upd, cur)
    if mlp_f:
        cur = cur + mlp(ln1(cur))
    loss = (cur * cs).sum()
    qv = None
    if q_f:
        qv = wq(ln2(cur))
        loss = loss + (qv * cq).sum()
    loss.backward()

    leaves = {k: v.double().clone().requires_grad_() for k, v in p.items()}
    upd2, h2 = upd0.double().requires_grad_(), h0.double().requires_grad_()
    out, q2 = sr.tail(upd2, h2, leaves, (gru_f, mlp_f, q_f))
    l2 = (out * cs).sum()
    if q_f:
        l2 = l2 + (q2 * cq).sum()
    l2.backward()
    assert _rel(out, cur) < TOL
    assert (q2 is None) == (qv is None)
    if q_f:
        assert _rel(q2, qv) < TOL
    assert _rel(h2.grad, h.grad) < TOL
    assert (upd2.grad is None) == (upd.grad is None) == (not gru_f)
    if gru_f:
        assert _rel(upd2.grad, upd.grad) < TOL
    live = 0
    for k in sr.PARAMS:
        assert (leaves[k].grad is None) == (named[k].grad is None), k
        if named[k].grad is not None:
            assert _rel(leaves[k].grad, named[k].grad) < TOL, k
            live += 1
    assert live == 4 * gru_f + 6 * mlp_f + 3 * q_f


@pytest.mark.parametrize("R", [17, 44])
@pytest.mark.parametrize("name", list(sr.FLAGS))
def test_stagewise_backward_is_autograd_of_the_chain(name, R):
    """The stage functions composed as the kernels compose them, nothing rounded: dupd, dh and the dY rows times their
    inputs (= the weight gradients) equal autograd on tail(); the summed per-block partials are the LayerNorm parameter
    gradients."""
    gru_f, mlp_f, q_f = flags = sr.FLAGS[name]
    p = sr.make_params()
    P = {k: v.double() for k, v in p.items()}
    upd, h = (t.double() for t in sr.make_rows(R))
    dout, dq = (t.double() for t in sr.make_grads(R))
    leaves = {k: v.clone().requires_grad_() for k, v in P.items()}
    upd_l, h_l = upd.clone().requires_grad_(), h.clone().requires_grad_()
    out, qv = sr.tail(upd_l, h_l, leaves, flags)
    loss = (out * dout).sum() + ((qv * dq).sum() if q_f else 0.0)
    loss.backward()
    want = {k: v.grad for k, v in leaves.items()}

    # forward, stage by stage
    cur = h
    if gru_f:
        gi, gh, _, _ = sr.gates(upd, h, P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"])
        hn = cur = sr.gru_out(gi, gh, h)[0]
    if mlp_f:
        y, mean1, rstd1, _, _ = sr.ln(hn, P["ln1_g"], P["ln1_b"])
        a = sr.fc1_relu(y, P["w1"], P["b1"])[0]
        cur = sr.fc2_res(a, P["w2"], P["b2"], hn)[0]
    if q_f:
        sn, mean2, rstd2, _, _ = sr.ln(cur, P["ln2_g"], P["ln2_b"])
    # backward
    got = {}
    ds = dout
    if q_f:
        got["wq"] = dq.t() @ sn
        ds, part2, _, mp = sr.ln_bwd(sr.dsn(dq, P["wq"])[0], cur, P["ln2_g"], mean2, rstd2, dout)
        assert part2.shape == (2, sr.blocks(R), D) and bool((mp >= part2.abs() * (1 - 1e-12)).all())
        got["ln2_g"], got["ln2_b"] = part2[0].sum(0), part2[1].sum(0)
    dhn = ds
    if mlp_f:
        dz = sr.dz(ds, P["w2"], a)[0]
        got["w2"], got["b2"] = ds.t() @ a, ds.sum(0)
        got["w1"], got["b1"] = dz.t() @ y, dz.sum(0)
        dhn, part1, _, _ = sr.ln_bwd(sr.dy1(dz, P["w1"])[0], hn, P["ln1_g"], mean1, rstd1, ds)
        got["ln1_g"], got["ln1_b"] = part1[0].sum(0), part1[1].sum(0)
    if gru_f:
        dgi, dgh, res, mgi, mgh, _ = sr.gate_bwd(gi, gh, h, dhn)
        assert bool((mgi >= dgi.abs() * (1 - 1e-12)).all()) and bool((mgh >= dgh.abs() * (1 - 1e-12)).all())
        got["w_ih"], got["b_ih"], got["w_hh"], got["b_hh"] = dgi.t() @ upd, dgi.sum(0), dgh.t() @ h, dgh.sum(0)
        assert _rel(sr.dupd(dgi, P["w_ih"])[0], upd_l.grad) < TOL
        dh = sr.dh(dgh, P["w_hh"], res)[0]
    else:
        dh = dhn
    assert _rel(dh, h_l.grad) < TOL
    assert set(got) == {k for k in sr.PARAMS if want[k] is not None}
    for k, v in got.items():
        assert _rel(v, want[k]) < TOL, k


def test_partials_are_per_block_and_see_only_their_rows():
    """Row r belongs to block r // 16 and to no other: moving one row's dy changes one block of the partials."""
    R = 33
    g = torch.Generator().manual_seed(0)
    dy, x = torch.randn(R, D, generator=g).double(), torch.randn(R, D, generator=g).double()
    gamma = torch.ones(D)
    _, mean, rstd, _, _ = sr.ln(x, gamma, torch.zeros(D))
    _, p0, _, _ = sr.ln_bwd(dy, x, gamma, mean, rstd)
    dy2 = dy.clone()
    dy2[32] += 1.0
    _, p1, _, _ = sr.ln_bwd(dy2, x, gamma, mean, rstd)
    assert p0.shape == (2, 3, D) and torch.equal(p0[:, :2], p1[:, :2]) and not torch.equal(p0[:, 2], p1[:, 2])
    assert torch.allclose(p1[1, 2], dy2[32]) and torch.allclose(p0[1, 0], dy[:16].sum(0))
    assert [sr.blocks(r) for r in (1, 15, 16, 17, 44, 352)] == [1, 1, 1, 2, 3, 22]


@pytest.mark.parametrize("R", sr.R_ALL)
def test_the_seeded_inputs_exercise_both_sides(R):
    c = sr.conditions(R)
    assert 0.2 <= c["zero_a"] <= 0.8, c
    assert c["open_gates"] >= 0.9, c
    assert c["min_var"] >= 1e-3, c


def test_magnitudes_bound_the_values():
    """mag >= |value| for every stage function (it is a sum of absolute terms of the same expression)."""
    R = 15
    P = {k: v.double() for k, v in sr.make_params().items()}
    upd, h = sr.make_rows(R)
    ok = lambda v, m: bool((m >= v.abs() * (1 - 1e-12)).all())
    gi, gh, mi, mh = sr.gates(upd, h, P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"])
    assert ok(gi, mi) and ok(gh, mh)
    hn, m = sr.gru_out(gi, gh, h)
    assert ok(hn, m)
    y, mean, rstd, m, mabs = sr.ln(hn, P["ln1_g"], P["ln1_b"])
    assert ok(y, m) and ok(mean, mabs)
    a, m = sr.fc1_relu(y, P["w1"], P["b1"])
    assert ok(a, m)
    s, m = sr.fc2_res(a, P["w2"], P["b2"], hn)
    assert ok(s, m)
    dx, part, m, mp = sr.ln_bwd(upd, hn, P["ln1_g"], mean, rstd, h)
    assert ok(dx, m) and ok(part, mp)
