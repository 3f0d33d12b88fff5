"""tests/space_ref.py checked without a GPU: the fp64 formula against a per-frame loop written differently, the rounding
model against the formula, the case table against the limits (the model stays inside them, every mutant of the model
leaves them by 2x) and against what it claims to cover."""
import pytest
import torch

import space_ref as sr


def _loop_reference(qkv, F, P, heads, cts):
    """attention.py:509-535 one (batch, head, frame) at a time: torch.softmax on an explicitly sliced frame."""
    B, N, C3 = qkv.shape
    C, S = C3 // 3, F * P
    x = qkv.double().requires_grad_()
    xt = torch.zeros(B, S, F, C, dtype=torch.float64)
    xd = torch.zeros(B, S, C, dtype=torch.float64)
    cls = torch.zeros(B, 1, C, dtype=torch.float64)
    xt_rows, cls_rows = [], []
    for b in range(B):
        for h in range(heads):
            c = slice(h * sr.HD, (h + 1) * sr.HD)
            q, k, v = x[b, :, :C][:, c], x[b, :, C:2 * C][:, c], x[b, :, 2 * C:][:, c]
            cls_rows.append((b, c, torch.softmax(q[:1] @ k.t() / 8.0, dim=-1) @ v))
            for f in range(F):
                kf, vf = k[1 + f * P:1 + (f + 1) * P], v[1 + f * P:1 + (f + 1) * P]
                xt_rows.append((b, f, c, torch.softmax(q[1:] @ kf.t() / 8.0, dim=-1) @ vf))
    loss = 0.0
    for b, c, o in cls_rows:
        cls[b, :, c] = o.detach()
        loss = loss + (o * cts[2].double()[b, :, c]).sum()
    for b, f, c, o in xt_rows:
        xt[b, :, f, c] = o.detach()
        xd[b, f * P:(f + 1) * P, c] = o.detach()[f * P:(f + 1) * P]
        loss = loss + (o * cts[0].double()[b, :, f, c]).sum() + (o[f * P:(f + 1) * P] * cts[1].double()[b, f * P:(f + 1) * P, c]).sum()
    loss.backward()
    return {"xt": xt, "xd": xd, "cls": cls, "dqkv": x.grad}


@pytest.fixture(scope="module")
def table():
    """Inputs and the fp64 reference of every row, computed once."""
    out = {}
    for c in sr.CASES:
        qkv, cts = sr.inputs(c)
        out[c[0]] = (qkv, cts, sr.space_exact(qkv, c[3], c[4], c[2], cts))
    return out


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (1, 2, 3, 1), (2, 1, 2, 5), (1, 3, 3, 7)])
def test_exact_matches_a_per_frame_loop(shape):
    B, heads, F, P = shape
    qkv, cts = sr.inputs(("loop%d_%d" % (F, P), B, heads, F, P))
    ref, loop = sr.space_exact(qkv, F, P, heads, cts), _loop_reference(qkv, F, P, heads, cts)
    for k in loop:
        assert float((ref[k] - loop[k]).abs().max()) <= 1e-12, k
    if P == 1:                                   # a one-key softmax: x~ is v, nothing reaches q or k from the patch rows
        C = heads * sr.HD
        assert float(ref["dqkv"][:, 1:, :C].abs().max()) == 0.0
        assert float(ref["mag_dq"].min()) > 0.0 and float(ref["mag_dk"].min()) > 0.0


def test_magnitudes_bound_the_exact_values(table):
    """Each magnitude is the same sum as its quantity with absolute values inside: it can only be larger."""
    for name, (_, _, ref) in table.items():
        C = ref["xd"].shape[-1]
        g = ref["dqkv"][:, 1:]
        for val, mag in ((ref["xt"], ref["mag_x"]), (ref["xd"], ref["mag_xd"]), (g[..., :C], ref["mag_dq"]),
                         (g[..., C:2 * C], ref["mag_dk"]), (g[..., 2 * C:], ref["mag_dv"])):
            assert bool((val.abs() <= mag * (1 + 1e-9) + 1e-300).all()), name


def test_rounded_with_rounding_off_is_exact(table):
    for c in sr.CASES:
        qkv, cts, ref = table[c[0]]
        off = sr.space_rounded(qkv, c[3], c[4], c[2], cts, rounding=False)
        for k in off:
            assert float((off[k] - ref[k]).abs().max()) <= 1e-12, (c[0], k)


def test_rounding_model_stays_inside_every_limit(table):
    """A statement about the table: on these inputs the kernels' own rounding points cost less than the limits."""
    worst = {}
    for c in sr.CASES:
        qkv, cts, ref = table[c[0]]
        got = sr.space_rounded(qkv, c[3], c[4], c[2], cts)
        for what, g, w, mag, lim, floor in sr.quantities(got, ref):
            x = sr.ratio(g, w, mag, floor)
            assert x <= lim, (c[0], what, x / sr.U, lim / sr.U)
            worst[what] = max(worst.get(what, 0.0), x / sr.U)
    print("\n".join("%-40s %.2f U" % kv for kv in worst.items()))


def test_every_mutant_leaves_a_limit_by_2x(table):
    """The limits detect what they are for: on every row, every wrong variant that applies puts some checked quantity
    at least 2x above its limit."""
    n = 0
    for c in sr.CASES:
        qkv, cts, ref = table[c[0]]
        for name, applies in sr.MUTANTS.items():
            if not applies(c):
                continue
            got = sr.space_rounded(qkv, c[3], c[4], c[2], cts, mutant=name)
            worst = max(sr.ratio(g, w, mag, floor) / lim for _, g, w, mag, lim, floor in sr.quantities(got, ref))
            assert worst >= 2.0, (c[0], name, worst)
            n += 1
    assert n >= 5 * len(sr.CASES)


def test_inputs_are_what_the_table_promises(table):
    for c in sr.CASES:
        _, B, heads, F, P = c
        qkv, cts, ref = table[c[0]]
        S, C = F * P, heads * sr.HD
        assert qkv.dtype == torch.bfloat16 and qkv.shape == (B, 1 + S, 3 * C)
        assert [tuple(t.shape) for t in cts] == [(B, S, F, C), (B, S, C), (B, 1, C)]
        assert B * heads * S * S * 8 < 64 << 20                       # the largest fp64 tensor of the reference
        if P < 3:
            continue
        q, k, _ = (sr._heads(t, heads) for t in qkv.double().split(C, dim=-1))
        A = torch.softmax(torch.einsum("bhsd,bhfpd->bhsfp", q[:, :, 1:], k[:, :, 1:].reshape(B, heads, F, P, sr.HD)) / 8.0, -1)
        spiked = A[:, :, 0:S - 1:3, :, P - 1]                         # mass on the frame's last real key
        assert 0.1 < float(spiked.median()) < 0.6, (c[0], float(spiked.median()))
        if sr.tiling(P)[1] > 1:                                       # the merge sees the largest logit first and last
            kr = sr.tiling(P)[0] * 32
            am = A[:, :, :S - 1].argmax(-1)
            first, last = float((am[:, :, 1::3] < kr).double().mean()), float((am[:, :, 0::3] >= (P - 1) // kr * kr).double().mean())
            assert first > 0.6 and last > 0.6, (c[0], first, last)      # most of each third, not every query
    assert sr.inputs(sr.CASES[3])[0].equal(table[sr.CASES[3][0]][0])  # seeded from the id alone


def test_table_covers_what_it_claims():
    ids = [c[0] for c in sr.CASES]
    assert len(set(ids)) == len(ids)
    routes = {c[0]: sr.route(c) for c in sr.CASES}
    for P in range(1, 449):                                           # the rule restated against its definition
        nkb, nt = sr.tiling(P)
        assert nkb * nt == (P + 31) // 32 and 1 <= nkb <= 7
        assert all(((P + 31) // 32) % k for k in range(nkb + 1, 8))
    # every pair the rule can produce for P <= 448: one tile with 1..7 blocks, and 8..14 blocks as 2x4, 3x3, 2x5, 11x1,
    # 2x6, 13x1, 2x7 -- (2, tiled) never occurs: a block count with largest divisor 2 would be 2 itself
    possible = {sr.tiling(P) for P in range(1, 449)}
    fwd_possible = {(nkb, nt > 1) for nkb, nt in possible}
    assert fwd_possible == {(k, False) for k in range(1, 8)} | {(k, True) for k in (1, 3, 4, 5, 6, 7)}
    assert {sr.tiling(c[4]) for c in sr.CASES} == possible
    assert {r["fwd"] for r in routes.values()} == fwd_possible
    assert {r["dq"] for r in routes.values()} == set(range(1, 15))
    assert {r["dkv"] for r in routes.values()} == set(range(1, 8))
    for nb in range(1, 15):                                           # batch strides and odd head counts at every block count
        rows = [c for c in sr.CASES if (c[4] + 31) // 32 == nb]
        assert any(c[1] >= 2 for c in rows) and any(c[2] in (1, 3) for c in rows), nb
        assert any(c[4] % 32 for c in rows), nb                       # and a ragged last block
    assert {1, 2, 3} <= {r["stream"] for r in routes.values()}        # dQ prologue: streams shorter than the ring
    assert {1, 2, 3} <= {r["chunks"] for r in routes.values()}        # dK/dV prologue
    for P in (1, 2, 31, 32, 33, 64, 65, 96, 97, 129, 160, 190, 196, 224, 225, 288, 300, 330, 352, 353, 384, 390, 416, 417,
              447, 448):
        assert any(c[4] == P for c in sr.CASES), P
    assert {(c[3], c[4]) for c in sr.CASES} >= {(1, 20), (1, 40), (1, 70), (16, 5), (16, 33), (5, 97)}
    S = {c[3] * c[4] for c in sr.CASES}
    assert {1, 30, 50, 90, 129} <= S and any(s % 128 == 0 for s in S)
    assert ("f16_p33", 1, 1, 16, 33) in sr.CASES
    grids = [g for r in routes.values() for g in r["grids"]]          # both branches of focus_xcd_group, and its even case
    assert any(g < 8 for g in grids) and any(g > 8 and g % 8 for g in grids) and any(g >= 8 and g % 8 == 0 for g in grids)
    assert all(c[3] <= sr.MAXF and c[4] <= 32 * sr.MAX_KEY_BLOCKS for c in sr.CASES)
    reached = sorted({("fwd", r["fwd"]) for r in routes.values()} | {("dq", r["dq"]) for r in routes.values()}
                     | {("dkv", r["dkv"]) for r in routes.values()}, key=str)
    print("kernel instantiations reached: %d\n%s" % (len(reached), reached))
    assert len(reached) == 13 + 14 + 7
