"""tests/attn_ref.py without a GPU: the plain attention and row softmax against torch's own in fp64, the hand-written
backward of the rounding model against autograd, and the conditions on the rows of CASES that make the GPU test's
tolerance a statement about the kernels (tests/test_gpu_attn_composed.py)."""
import pytest
import torch
import torch.nn.functional as F

import attn_ref as ar

SMALL = [  # B, heads, Nq, Nk, d, causal
    (2, 3, 7, 7, 8, True),
    (1, 2, 9, 4, 5, False),
    (3, 1, 1, 6, 16, False),
]


def _small(B, heads, Nq, Nk, d, seed=0):
    g = torch.Generator().manual_seed(seed + Nq + 3 * Nk)
    C = heads * d
    q, k, v, cu = (torch.randn(B, n, C, generator=g, dtype=torch.float64) for n in (Nq, Nk, Nk, Nq))
    return q, k, v, cu


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert ar.err(a, b) <= tol, ar.err(a, b)


@pytest.mark.parametrize("B,heads,Nq,Nk,d,causal", SMALL)
def test_attention_is_torch_sdpa(B, heads, Nq, Nk, d, causal):
    q, k, v, cu = _small(B, heads, Nq, Nk, d)
    scale = d ** -0.5
    got = ar.attention(q, k, v, heads, scale, causal, None, cu)
    qd, kd, vd = (t.clone().requires_grad_() for t in (q, k, v))
    split = lambda t: t.view(B, t.shape[1], heads, d).transpose(1, 2)
    mask = torch.tril(torch.ones(Nq, Nk, dtype=torch.bool)) if causal else None
    o = F.scaled_dot_product_attention(split(qd), split(kd), split(vd), attn_mask=mask, scale=scale)
    o = o.transpose(1, 2).reshape(B, Nq, heads * d)
    (o * cu).sum().backward()
    for a, b in zip(got, (o.detach(), qd.grad, kd.grad, vd.grad)):
        _close(a, b)


@pytest.mark.parametrize("causal", [False, True])
def test_attention_with_a_multiplier_is_the_einsum_formula(causal):
    B, heads, N, d = 2, 2, 6, 4
    q, k, v, cu = _small(B, heads, N, N, d, seed=5)
    g = torch.Generator().manual_seed(9)
    drop = torch.bernoulli(torch.full((B, heads, N, N), 0.75), generator=g).double() / 0.75
    scale = 0.3
    got = ar.attention(q, k, v, heads, scale, causal, drop, cu)
    qd, kd, vd = (t.clone().requires_grad_() for t in (q, k, v))
    q4, k4, v4 = (t.view(B, N, heads, d) for t in (qd, kd, vd))
    s = scale * torch.einsum("bqhd,bkhd->bhqk", q4, k4)
    if causal:
        s = s + torch.triu(torch.full((N, N), float("-inf"), dtype=torch.float64), diagonal=1)
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1) * drop, v4).reshape(B, N, heads * d)
    (o * cu).sum().backward()
    for a, b in zip(got, (o.detach(), qd.grad, kd.grad, vd.grad)):
        _close(a, b)


@pytest.mark.parametrize("scale", [1.0, 48 ** -0.5, -0.37])
def test_softmax_rows_is_torch_softmax(scale):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4, 5, 13, generator=g, dtype=torch.float64) * 30).requires_grad_()
    dy = torch.randn(4, 5, 13, generator=g, dtype=torch.float64)
    y = torch.softmax(scale * x, -1)
    y.backward(dy)
    _close(ar.softmax_rows(x.detach(), scale), y.detach())
    _close(ar.softmax_rows_bwd(dy, y.detach(), scale), x.grad)
    assert torch.equal(ar.softmax_rows(torch.full((3, 9), 2.5), scale), torch.full((3, 9), 1.0 / 9, dtype=torch.float64))


@pytest.mark.parametrize("period,L", [(1, 1), (5, 5), (11, 11), (11, 14), (11, 7)])
def test_softmax_rows_period_masks_the_tail_to_exact_zero(period, L):
    g = torch.Generator().manual_seed(period + L)
    rows = 3 * period + 2
    x = torch.randn(rows, L, generator=g, dtype=torch.float64) * 4
    hidden = torch.arange(L)[None, :] > (torch.arange(rows) % period)[:, None]
    x[hidden] = 1e30                                                       # must reach neither the maximum nor the sum
    y = ar.softmax_rows(x.view(rows, 1, L), 0.7, period).view(rows, L)     # rows are counted over all leading axes
    assert (y[hidden] == 0).all() and not torch.signbit(y[hidden]).any()
    for r in range(rows):
        n = min(L, r % period + 1)
        _close(y[r, :n], torch.softmax(0.7 * x[r, :n], -1))
    _close(y.sum(-1), torch.ones(rows, dtype=torch.float64))


@pytest.mark.parametrize("B,heads,Nq,Nk,d,causal", SMALL)
@pytest.mark.parametrize("dropped", [False, True])
def test_unrounded_model_is_the_formula(B, heads, Nq, Nk, d, causal, dropped):
    """attention_rounded's backward is written by hand: with no rounding it must be autograd's."""
    q, k, v, cu = _small(B, heads, Nq, Nk, d, seed=11)
    drop = None
    if dropped:
        g = torch.Generator().manual_seed(2)
        drop = torch.bernoulli(torch.full((B, heads, Nq, Nk), 0.8), generator=g).double() / 0.8
    want = ar.attention(q, k, v, heads, d ** -0.5, causal, drop, cu)
    got = ar.attention_rounded(q, k, v, heads, d ** -0.5, causal, drop, cu, torch.float64)
    for a, b in zip(got, want):
        _close(a, b)


def test_round_trip_is_the_storage_format():
    x = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -25, 1e-3], dtype=torch.float64)
    assert torch.equal(ar.rt(x, torch.float64), x)
    assert ar.rt(x, torch.bfloat16).tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0, float(torch.tensor(1e-3).bfloat16())]
    assert ar.rt(x, torch.float32).tolist() == [1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0, float(torch.tensor(1e-3))]


def test_case_table_is_the_one_the_composed_route_is_held_to():
    assert len(ar.CASES) == 9 and len({ar.case_id(c) for c in ar.CASES}) == 9
    assert ar.FLOOR == {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -6}
    assert ar.CAP == {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -4}
    assert ar.FACTOR >= 4 and ar.FACTOR == 2 ** round(torch.log2(torch.tensor(ar.FACTOR)).item())
    for c in ar.CASES:
        assert 0 < c["gain"] <= 0.7


@pytest.mark.parametrize("case", ar.CASES, ids=ar.case_id)
def test_case_is_well_conditioned(case):
    """A condition on the inputs, so that it binds the reference and not the kernel: the rounding model of every row
    stays inside CAP, which therefore can never be what lets a GPU case pass."""
    q, k, v, cu, drop, scale = ar.inputs(case)
    dt, heads, causal = case["dtype"], case["heads"], case["causal"]
    for t in (q, k, v, cu) + (() if drop is None else (drop,)):
        assert t.dtype == dt and torch.isfinite(t).all()
    assert case["Nk"] >= 1 and (not causal or case["Nq"] == case["Nk"])     # every query sees at least one key
    if drop is not None:
        assert set(drop.unique().tolist()) == {0.0, float(torch.tensor(1 / (1 - case["p"])).to(dt))}
        assert abs(float((drop == 0).double().mean()) - case["p"]) < 0.01
    exact = ar.attention(q, k, v, heads, scale, causal, drop, cu)
    model = ar.attention_rounded(q, k, v, heads, scale, causal, drop, cu, dt)
    for name, m, e in zip(("out", "dq", "dk", "dv"), model, exact):
        assert torch.isfinite(e).all() and float(e.abs().max()) > 0
        bound = ar.FACTOR * ar.err(m, e)
        print("%-40s %-3s err(model, exact) %.3e  FACTOR * err %.3e  cap %.3e" % (ar.case_id(case), name, ar.err(m, e), bound, ar.CAP[dt]))
        assert bound <= ar.CAP[dt], "%s: %.3e" % (name, bound)
