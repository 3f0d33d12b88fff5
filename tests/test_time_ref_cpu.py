"""tests/time_ref.py checked without a GPU: the fp64 formula against a per-(b, s, h) loop written differently, the stage
chain against the formula (the re-association u = Wk^T q2), the rounding model against the limits on every row of the
tables, every mutant of the model against the limits, the restated dispatch exhaustively, and the tables against what
they claim to reach."""
import numpy as np
import pytest
import torch

import time_ref as tr

SMALL = 120               # rows: the mutants and the loop run on the rows of the table up to this size


def _loop_reference(q2, xt, wk, bk, cls, ct, heads):
    """attention.py:536-549 one (batch, query, head) at a time, with torch.softmax on an explicit [F] vector."""
    B, S, F, C = xt.shape
    Q, X, W, Bk = (t.double().clone().requires_grad_() for t in (q2, xt, wk, bk))
    loss, o = 0.0, torch.zeros(B, 1 + S, C, dtype=torch.float64)
    o[:, 0] = cls.double()[:, 0]
    for b in range(B):
        for s in range(S):
            for h in range(heads):
                c = slice(h * tr.HD, (h + 1) * tr.HD)
                keys = X[b, s] @ W[c].t() + Bk[c]                                     # [F, 64]
                p = torch.softmax(keys @ Q[b, s, c] / 8.0, dim=0)
                row = p @ X[b, s][:, c]
                o[b, 1 + s, c] = row.detach()
                loss = loss + (row * ct.double()[b, 1 + s, c]).sum()
    loss.backward()
    R = B * S
    return {"out_cat": o, "dq2": Q.grad.reshape(R, C), "dxt": X.grad.reshape(R, F, C), "dwk": W.grad, "dbk": Bk.grad}


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


@pytest.fixture(scope="module")
def table():
    """Inputs, the flat dict, the fp64 reference and the rounding model of every row, computed once."""
    res = {}
    for c in tr.CASES:
        q2, xt, wk, bk, cls, ct = tr.inputs(c)
        inp = tr.flat(c, q2, xt, wk, ct)
        ex = tr.time_exact(q2, xt, wk, bk, cls, ct, c[4])
        res[c[0]] = (inp, ex, tr.time_rounded(inp["q2"], inp["xt"], wk, inp["dout"], c[4]))
    return res


@pytest.mark.parametrize("shape", [(1, 3, 4, 1), (2, 2, 8, 3), (1, 2, 16, 2)])
def test_exact_matches_a_per_row_loop(shape):
    B, S, F, heads = shape
    case = ("loop_%d_%d" % (F, heads), B, S, F, heads, "C", 0, "unit")
    args = tr.inputs(case)
    ex, loop = tr.time_exact(*args, heads), _loop_reference(*args, heads)
    for k in loop:
        assert _close(ex[k], loop[k]), k
    assert torch.equal(ex["out_cat"][:, 0], args[4].double()[:, 0])               # row 0 = cls
    assert torch.equal(ex["dcls"], args[5].double()[:, :1])


def test_bias_gets_no_gradient(table):
    """The softmax over the frames is shift invariant: d bk == 0 is a property of the original form, to rounding."""
    for name, (inp, ex, _) in table.items():
        assert float(ex["dbk"].abs().max()) <= 1e-12 * (1.0 + float(ex["dwk"].abs().max())), name
    c = tr.CASES[2]
    q2, xt, wk, bk, cls, ct = tr.inputs(c)
    other = tr.time_exact(q2, xt, wk, bk * 0 + 3.0, cls, ct, c[4])
    for k in ("attn", "out", "dxt", "dq2", "dwk"):
        assert _close(other[k], table[c[0]][1][k]), k


def test_stage_chain_reproduces_the_exact_form(table):
    """u = Wk^T q2, logits, softmax, out, dl, g, dx~, dq2, dWk composed = the original form and its autograd gradients."""
    for name, (inp, ex, _) in table.items():
        q2, xt, wk, dout = inp["q2"], inp["xt"], inp["wk"], inp["dout"]
        u_ = tr.u(q2, wk)
        a = tr.attn(tr.logits(u_, xt))
        dl_ = tr.dl(a, dout, xt)
        g_ = tr.g(dl_, xt)
        chain = {"attn": a, "out": tr.out(a, xt), "dl": dl_, "g": g_, "dxt": tr.dxt(a, dl_, dout, u_), "dq2": tr.dq2(g_, wk),
                 "dwk": tr.dwk(q2, g_)}
        for k, v in chain.items():
            assert _close(v, ex[k]), (name, k)
        if inp["xt"].shape[0] <= SMALL:
            off = tr.time_rounded(q2, xt, wk, dout, inp["heads"], rounding=False)
            for k in chain:
                assert _close(off[k], ex[k]), (name, k, "rounding off")


def test_magnitudes_bound_their_quantities(table):
    for name, (inp, ex, _) in table.items():
        q2, xt, wk, dout = inp["q2"], inp["xt"], inp["wk"], inp["dout"]
        a, xa, ua = ex["attn"], inp["xt"].double().abs(), tr.u(q2, wk).abs()
        mdl = tr.mag_dl(a, dout, xt)
        pairs = [(ex["out"], tr.out(a, xa)), (ex["dl"], mdl), (ex["g"], tr.g(ex["dl"].abs(), xa)),
                 (tr.g(ex["dl"].abs(), xa), tr.g(mdl, xa)),
                 (ex["dxt"], tr._adout(a, dout) + torch.einsum("rhf,rhc->rfc", ex["dl"].abs(), ua)),
                 (ex["dq2"], tr.dq2(ex["g"].abs(), wk.double().abs())), (ex["dwk"], tr.dwk(q2.double().abs(), ex["g"].abs()))]
        for i, (val, mag) in enumerate(pairs):
            assert bool((val.abs() <= mag * (1 + 1e-9) + 1e-300).all()), (name, i)


def test_rounding_model_stays_inside_every_limit(table):
    """A statement about the tables: on these inputs the kernels' own rounding points cost less than the limits -- every
    element of every quantity, stage by stage and end to end."""
    worst = {}
    for c in tr.CASES:
        inp, ex, got = table[c[0]]
        rows = tr.quantities(inp, got, ex) + tr.gw_quantities(got["g"], inp["q2"], inp["wk"], got)
        for what, g, w, mag, lim in rows:
            assert g.shape == w.shape == mag.shape, (c[0], what)
            x = tr.ratio(g, w, mag)
            assert x <= lim, (c[0], what, x / tr.U, lim / tr.U)
            worst[what] = max(worst.get(what, 0.0), x / lim)
        assert float(got["dl16"][:, :, c[4]:].abs().max() if c[4] < tr.MAXH else 0.0) == 0.0
    for c in tr.GW_CASES:
        g_, q2, wk = tr.gw_inputs(c)
        for what, g, w, mag, lim in tr.gw_quantities(g_, q2, wk, tr.gw_rounded(g_, q2, wk)):
            x = tr.ratio(g, w, mag)
            assert x <= lim, (c[0], what, x, lim)
            worst[what] = max(worst.get(what, 0.0), x / lim)
    print("\n".join("%-28s %.3f of its limit" % kv for kv in worst.items()))


def test_expf_needs_no_term_of_its_own(table):
    """__expf's share of a probability's error (time_ref.EXPF_REL, counted from its argument range) is inside the 1 %
    allowance of the attn2 limit on every element of every row."""
    low = float("inf")
    for name, (inp, ex, _) in table.items():
        u_ = tr.u(inp["q2"], inp["wk"])
        A = tr.mag_attn(ex["attn"], u_, inp["xt"])
        rel = A / ex["attn"].clamp_min(1e-300)                                       # Ebar_f + sum a Ebar
        rel = rel[ex["attn"] > 1e-200]
        low = min(low, float(rel.min()))
        assert 0.01 * tr.U * float(rel.min()) >= tr.EXPF_REL, (name, float(rel.min()))
    print("smallest Ebar_f + sum a Ebar of the table: %.2f" % low)


def test_every_mutant_leaves_a_limit_by_2x(table):
    """The limits detect what they are for.  A mutant that no row catches means a row is missing from the table."""
    caught = {m: [] for m in tr.MUTANTS}
    gw_only = ("dwk_last_tile_missing", "dq2_tile_from_previous")
    for c in tr.CASES:
        inp, ex, _ = table[c[0]]
        R, F, _ = inp["xt"].shape
        if R > SMALL:
            continue
        for name, applies in tr.MUTANTS.items():
            if name in gw_only or not applies(c[4], F, R):
                continue
            got = tr.time_rounded(inp["q2"], inp["xt"], inp["wk"], inp["dout"], c[4], mutant=name)
            worst = max(tr.ratio(g, w, mag) / lim for _, g, w, mag, lim in tr.quantities(inp, got, ex))
            if name == "dl_pad_nonzero":
                assert float(got["dl16"][:, :, c[4]:].abs().max()) > 0.0           # what the GPU test's +0 assertion sees
            if worst >= 2.0:
                caught[name].append(c[0])
    for c in tr.GW_CASES:
        g_, q2, wk = tr.gw_inputs(c)
        for name in gw_only:
            if not tr.MUTANTS[name](tr.GW_HEADS, 0, c[1]):
                continue
            got = tr.gw_rounded(g_, q2, wk, mutant=name)
            if max(tr.ratio(g, w, mag) / lim for _, g, w, mag, lim in tr.gw_quantities(g_, q2, wk, got)) >= 2.0:
                caught[name].append(c[0])
    print("\n".join("%-26s caught on %d rows" % (m, len(r)) for m, r in caught.items()))
    for m, rows in caught.items():
        assert rows, m
    # the unit-scale rows catch every mutant that applies to them: nothing rests on one lucky row
    for c in tr.CASES:
        R = c[1] * c[2]
        if c[7] == "unit" and 32 <= R <= SMALL:
            for name, applies in tr.MUTANTS.items():
                if name not in gw_only and applies(c[4], c[3], R):
                    assert c[0] in caught[name], (c[0], name)
    assert all(len(caught[m]) >= 5 for m in gw_only)


def test_owner_tables_and_ring_turns_exhaustively():
    """owner_of_block (both tables) hands every (chunk, range) to exactly one workgroup; turn_begin cuts the tiles into
    contiguous whole turns: every (chunk, tile) below ntiles has exactly one owner, no range starts past its end, and the
    tiles run past ntiles are fewer than one ring depth, all in the last non-empty range."""
    seen = set()
    for heads in range(1, tr.MAXH + 1):
        for spread in (False, True):
            table, nranges = tr.owners(heads, spread)
            assert len(table) == tr.GRID and nranges >= 1
            live = [t for t in table if t is not None]
            assert sorted(live) == [(cc, r) for cc in range(heads) for r in range(nranges)], (heads, spread)
            if not spread:                                       # the owners of a range sit on at most ceil(nchunk / g) XCDs
                gdiv = max(dv for dv in range(1, 9) if heads % dv == 0)
                for r in range(nranges):
                    xcds = {i & 7 for i, t in enumerate(table) if t is not None and t[1] == r}
                    assert len(xcds) <= heads // gdiv, (heads, r)
            if nranges in seen:
                continue
            seen.add(nranges)
            rng = np.arange(nranges + 1, dtype=np.int64)
            for depth in (2, 3):
                for ntiles in range(1, 601):
                    turns = (ntiles + depth - 1) // depth
                    begins = (turns * rng // nranges) * depth
                    assert [tr.turn_begin(ntiles, r, nranges, depth) for r in (0, nranges // 2, nranges)] == \
                        [begins[0], begins[nranges // 2], begins[-1]]
                    assert begins[0] == 0 and bool((np.diff(begins) >= 0).all()) and bool((begins % depth == 0).all())
                    owner_count = np.zeros(begins[-1], dtype=np.int64)            # tiles 0 .. end: who runs them
                    np.add.at(owner_count, np.concatenate([np.arange(b, e) for b, e in zip(begins[:-1], begins[1:])]), 1)
                    assert bool((owner_count == 1).all())
                    past = begins[-1] - ntiles
                    assert 0 <= past < depth
                    last = max(r for r in range(nranges) if begins[r + 1] > begins[r])
                    assert begins[last + 1] == begins[-1] and begins[last] <= ntiles - 1   # ... and it owns a real tile too
    assert len(seen) >= 12


def test_route_instances_are_the_dispatch():
    """The staged / direct choice restated against the LDS sizes and the exclusions of the two dispatchers."""
    assert tr.lds_staged_fwd(12, 8) == 142336                    # "139 KB for 12 heads, F = 8"
    for F in (4, 8, 16):
        for heads in range(1, 17):
            (fi, fd), (bi, bd) = tr.instances(heads, F)
            w = tr.upw_of(heads)
            assert 1 <= w <= 4 and (w - 1) * 4 < heads <= w * 4
            assert ("lds" in fi) == (F <= 8 and not (F == 8 and heads >= 15)), (F, heads)
            assert ("lds" in bi) == (not (w == 4 and F != 8)), (F, heads)
            assert fd == (2 if "lds" in fi else 3) and bd == (2 if "lds" in bi or F == 16 else 3)
            (fi0, fd0), (bi0, bd0) = tr.instances(heads, F, lds=False)
            assert "lds" not in fi0 + bi0 and fd0 == 3 and bd0 == (2 if F == 16 else 3)
    assert len(tr.reachable_instances()) == 25
    assert len(tr.reachable_instances(lds=False) - tr.reachable_instances()) == 17   # only under FOCUS_T2_LDS=0


def test_gw_route():
    for R in range(32, 32 * 700, 32):
        r = tr.gw_route(R)
        assert r["splits"] == min(r["tiles"], 21) and r["used"] <= r["splits"]
        assert (r["used"] - 1) * r["tiles_per_split"] + r["last"] == r["tiles"] and 1 <= r["last"] <= r["tiles_per_split"]
    pat = {c[1]: tr.gw_route(c[1]) for c in tr.GW_CASES}
    assert (pat[32]["used"], pat[32]["tiles_per_split"]) == (1, 1) and (pat[64]["used"], pat[64]["tiles_per_split"]) == (2, 1)
    assert (pat[672]["used"], pat[672]["tiles_per_split"], pat[672]["last"]) == (21, 1, 1)      # one tile per split
    assert (pat[704]["used"], pat[704]["tiles_per_split"], pat[704]["last"]) == (11, 2, 2)      # two per split, 11 used
    assert (pat[736]["used"], pat[736]["tiles_per_split"], pat[736]["last"]) == (12, 2, 1)      # the last split owns one
    assert (pat[1376]["used"], pat[1376]["tiles_per_split"], pat[1376]["last"]) == (15, 3, 1)   # three per split
    assert {c[2] for c in tr.GW_CASES} == {768, 776}
    assert [c[1] for c in tr.GW_CASES] == [32, 64, 672, 704, 736, 1376]


def test_table_reaches_what_it_claims():
    ids = [c[0] for c in tr.CASES]
    assert len(set(ids)) == len(ids)
    routes = {c[0]: tr.route(c) for c in tr.CASES}
    reached = {r[k]["instance"] for r in routes.values() for k in ("fwd", "bwd")}
    print("instances reached: %d\n%s" % (len(reached), "\n".join(sorted(reached))))
    assert reached == tr.reachable_instances() and len(reached) == 25
    # the direct instances and the second owner table, as the child processes of the GPU test reach them
    off = {tr.route(c, lds=False)[k]["instance"] for c in tr.CASES for k in ("fwd", "bwd")}
    assert off == tr.reachable_instances(lds=False) and len(off - reached) == 17
    for never in ("time2_logits_lds_kernel<4,2>", "time2_logits_lds_kernel<4,4>", "time2_logits_lds_kernel<8,4>",
                  "time2_logits_kernel<16,2>", "time2_logits_kernel<16,3>", "time2_dx_lds_kernel<4,2>",
                  "time2_dx_lds_kernel<16,2>", "time2_dx_lds_kernel<16,3>", "time2_dx_kernel<4,4>"):
        assert never in reached, never
    by = lambda F, heads: [c for c in tr.CASES if c[3] == F and c[4] == heads]
    assert by(8, 14) and by(8, 15)                                # the staged / direct boundary of the logits kernel
    assert "lds" in routes[by(8, 14)[0][0]]["fwd"]["instance"] and "lds" not in routes[by(8, 15)[0][0]]["fwd"]["instance"]
    assert {1, 15, 16, 17} <= {r["rows"] for r in routes.values()}
    assert any(r["ntiles"] < r["nranges"] and r["fwd"]["empty"] > 0 for r in routes.values())
    whole = [c for c in tr.CASES if all(routes[c[0]]["rows"] % (routes[c[0]]["nranges"] * routes[c[0]][k]["depth"] * 16) == 0
                                        for k in ("fwd", "bwd"))]
    assert whole
    for c in whole:                                               # ... and the same count plus one row
        r = routes[c[0]]
        assert r["fwd"]["past"] == 0 and r["fwd"]["empty"] == 0
        plus = [d for d in tr.CASES if d[3:5] == c[3:5] and d[1] * d[2] == r["rows"] + 1]
        assert plus and routes[plus[0][0]]["fwd"]["past"] > 0
    assert any(r[k]["most_turns"] >= 2 for r in routes.values() for k in ("fwd", "bwd"))
    assert any(r["fwd"]["depth"] == 3 and r["fwd"]["past"] == 2 for r in routes.values())     # a ring's worth of clamped tiles
    assert any(c[1] == 1 and c[2] % 16 for c in tr.CASES)
    assert any(c[1] == 3 and c[2] % 16 and c[2] > 16 for c in tr.CASES)                       # a tile straddles a batch boundary
    assert {c[5] for c in tr.CASES} == {"C", "C+8", "2C"}
    assert any(c[6] == 0 for c in tr.CASES) and any(c[6] > 0 and c[6] % 8 == 0 for c in tr.CASES)
    assert all(c[6] % 8 == 0 for c in tr.CASES)
    for F in (4, 8, 16):
        assert {tr.upw_of(c[4]) for c in tr.CASES if c[3] == F} == {1, 2, 3, 4}, F
    assert {1, 3, 4, 5, 8, 9, 11, 12, 13, 16} <= {c[4] for c in tr.CASES}
    assert sum(1 for c in tr.CASES if c[4] == 1) >= 3                                         # the dl padding of one head
    assert {c[7] for c in tr.CASES} == {"unit", "peaked", "big"}
    assert max(r["rows"] for r in routes.values()) <= 4096
    assert tr.inputs(tr.CASES[3])[0].equal(tr.inputs(tr.CASES[3])[0])


def test_inputs_are_what_the_table_promises(table):
    for c in tr.CASES:
        inp, ex, _ = table[c[0]]
        _, B, S, F, heads = c[:5]
        assert inp["q2"].dtype == inp["xt"].dtype == inp["wk"].dtype == torch.bfloat16
        assert inp["xt"].shape == (B * S, F, heads * tr.HD) and inp["dout"].shape == (B * S, heads * tr.HD)
        lg = tr.logits(tr.u(inp["q2"], inp["wk"]), inp["xt"])
        spread = (lg.max(-1).values - lg.min(-1).values)
        if c[7] == "unit":
            assert 1.0 < float(spread.median()) < 6.0, (c[0], float(spread.median()))
        elif c[7] == "big":
            assert float(lg.abs().max()) > 60.0 and float(spread.median()) > 60.0, c[0]
        else:
            top = ex["attn"][0::3].max(-1).values
            assert float(top.min()) > 0.99, (c[0], float(top.min()))                          # near one-hot
            assert 1.0 < float(spread[1::3].median()) < 6.0
