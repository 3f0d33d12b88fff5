"""The k2-free temporal step of trajectory attention (csrc/traj_time2.hip, csrc/traj_time2_gw.hip; bf16, head dim 64)
written plainly in fp64, a model of where those kernels round, the magnitudes and counted limits they are held to, the
dispatch restated (kernel instance, owner table, ring turns), the case tables, and wrong variants of the model.  The checker
of tests/test_gpu_traj_time2.py, itself checked without a GPU by tests/test_time_ref_cpu.py; the product never imports
this, and this imports neither a GPU nor focus_amd.  Every function works on the device of its arguments.

  time_exact       attention.py:536-549 in its original form (k2 = x~ Wk^T + bk) in fp64, gradients by autograd
  u .. dwk         the re-associated chain (u = Wk[h]^T q2) one stage at a time, each on the inputs it is given
  time_rounded     the chain with a bf16 round trip exactly where the kernels round
  quantities       the checked parts of a result: stage by stage, and end to end against time_exact
  route / gw_route what the dispatchers pick for a row
  CASES / GW_CASES / inputs / gw_inputs,  MUTANTS

Flat layouts (R = B S rows): q2, dout [R,C]; x~, dx~ [R,F,C]; u [R,h,C]; logits, attn, da, dl [R,h,F]; g [h,R,C];
Wk [C (h,dd), C (c)].  dl here INCLUDES the factor scale: dl = d(loss)/d(u . x~).

Where the kernels round to bf16 (traj_time2.hip unless named; line numbers as of the commit that added this file):
  u        compute_u_tile, :204 `p.e[r] = f32_to_bf16(acc[r])`: the operand of the logit product AND of the dx~ product
  logits   fp32: per-chunk partials :338 / :515 `slab[...] = o` (direct / staged kernel), summed in time2_softmax_kernel;
           softmax fp32 with __expf (:547); attn2 stored fp32 (:552)
  out      time2_out_kernel, :581 `... = pack8(o)`: once
  dl       time2_dlg_kernel: :621 `sdl[rl][f][h] = scale * a[f] * (da[f] - dot)` in fp32, used in fp32 for g; stored to HBM
           as bf16 (:639 `dl + ... = pack8(v)`) for the dx kernels
  g        time2_dlg_kernel, :654 `gout + ... = pack8(g8)`: once
  dx~      time2_dx_kernel :793-794 / time2_dx_lds_kernel :985-986, `v = fmaf(av, dv, acc)`, `o[i][0] = pack8(v)`:
           a dout + sum_h dl_bf16 u_bf16, once
  dq2      traj_time2_gw.hip:130 `o[...] = f32_to_bf16(accq[r])` (or the batched GEMM's output): once
  dWk      fp32 throughout (traj_time2_gw.hip:141 accumulates, :155 stores, time2_gw_reduce_kernel sums the splits)

Limits.  Every bf16 rounding costs at most U = 2^-8 of its magnitude; 1 % is the allowance for fp32 summation order.  A
quantity is held to  |got - want| <= limit * magnitude  per element, with the UNCANCELLED magnitude:
  attn2    1 rounding (u), carried through the softmax to first order: Ebar = scale sum_c |x~||u| per logit,
           magnitude a_f (Ebar_f + sum_f' a_f' Ebar_f').  __expf: the argument l - max is <= 0, and below -88 the result is
           under fp32's normal range (TINY covers it); v_exp_f32 is good to 1 ulp and the argument's scaling by log2(e)
           costs |arg| 2^-24 relative, so a numerator is off by at most (88 + 3) 2^-23 relative and the denominator by as
           much: EXPF_REL.  test_time_ref_cpu.py shows EXPF_REL to lie inside the 1 % on every element of every row of
           the table (it needs Ebar_f + sum a Ebar >= 0.56; the table's smallest is ~5), so it gets no term of its own
  out      1: magnitude sum_f a |x~|
  dl       1: magnitude scale a_f (|da_f| + sum_f' a_f' |da_f'|)  (the cancellation da - sum a da happens in fp32)
  g        1: magnitude sum_f mag_dl |x~|   (fp32 dl inside the kernel: the output rounding only)
  dx~      2 (u as the operand, the output): magnitude a |dout| + sum_h |dl||u|
  dq2      1, plus the fp32 chain over K = 768: magnitude |dq2| + (FP32_CHAIN / limit) sum_c |g||Wk|
  dWk      fp32 chain: FP32_CHAIN sum_r |q2||g|  (the figure tests/test_gpu_kernels.py holds the same kernel to)
End to end against time_exact the magnitudes add up, one term per rounding that reaches the quantity (first order):
  P_f = scale (A_f (|da_f| + sum a|da|) + a_f sum_f' A_f' |da_f'|),  A = the attn2 magnitude   (what attn2's error does to dl)
  out      sum_f a|x~| + sum_f A_f |x~|
  g        sum_f (mag_dl + P) |x~|
  dx~      A |dout| + sum_h (mag_dl + P) |u|  +  sum_h |dl||u|  +  a|dout| + sum_h |dl||u|
These are constants counted from the list above, not fitted to a GPU result.  Every magnitude gets TINY = 2^-100 added:
below fp32's normal range (2^-126) results may flush to zero.
"""
import zlib

import torch

U = 2.0 ** -8
LIM_ATT = 1.01 * U
LIM_OUT = 1.01 * U
LIM_DL = 1.01 * U
LIM_G = 1.01 * U
LIM_DX = 2.02 * U
LIM_DQ2 = 1.01 * U
LIM_E2E = 1.01 * U
FP32_CHAIN = 2e-6
TINY = 2.0 ** -100
EXPF_REL = 2 * (88 + 3) * 2.0 ** -23   # __expf's share of a probability's relative error (see above)
HD = 64
MAXH = 16
TQ = 16                   # queries per tile of the chunk-owner kernels
LDS_MAX = 160 * 1024
GRID = 256
GW_C, GW_HEADS, GW_TR = 768, 12, 32


def r16(t):
    """Round trip of fp64 values through bf16 (round to nearest even)."""
    return t.float().bfloat16().double()


def _same(t):
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the formula
# ---------------------------------------------------------------------------------------------------------------------
def time_exact(q2, xt, wk, bk, cls, ct, heads):
    """attention.py:536-549 in fp64: q2 [B,S,C], x~ [B,S,F,C], Wk [C,C], bk [C], cls [B,1,C], cotangent ct [B,1+S,C].
    -> dict (flat layouts): out_cat [B,1+S,C]; attn, out, dl, g; dq2, dxt, dwk, dbk, dcls by autograd."""
    B, S, F, C = xt.shape
    R, scale = B * S, HD ** -0.5
    Q, X, W, Bk, CL = (t.double().clone().requires_grad_() for t in (q2, xt, wk, bk, cls))
    k2 = (X @ W.t() + Bk).reshape(B, S, F, heads, HD)
    logit = torch.einsum("bshd,bsfhd->bshf", Q.reshape(B, S, heads, HD) * scale, k2)
    logit.retain_grad()
    A = torch.softmax(logit, dim=-1)
    o = torch.einsum("bshf,bsfhd->bshd", A, X.reshape(B, S, F, heads, HD)).reshape(B, S, C)
    cat = torch.cat([CL, o], 1)
    (cat * ct.double()).sum().backward()
    dl_ = (logit.grad * scale).reshape(R, heads, F)
    return {"out_cat": cat.detach(), "attn": A.detach().reshape(R, heads, F), "out": o.detach().reshape(R, C), "dl": dl_,
            "g": torch.einsum("rhf,rfc->hrc", dl_, xt.double().reshape(R, F, C)),
            "dq2": Q.grad.reshape(R, C), "dxt": X.grad.reshape(R, F, C), "dwk": W.grad, "dbk": Bk.grad, "dcls": CL.grad}


# ---------------------------------------------------------------------------------------------------------------------
# the re-associated chain, one stage at a time (fp64, each on what it is given)
# ---------------------------------------------------------------------------------------------------------------------
def _wkh(wk):
    C = wk.shape[1]
    return wk.double().reshape(C // HD, HD, C)


def _xh(xt, heads):
    R, F, C = xt.shape
    return xt.double().reshape(R, F, heads, HD)


def u(q2, wk):
    """u[r,h,c] = sum_dd Wk[h*64+dd, c] q2[r, h*64+dd]"""
    wkh = _wkh(wk)
    return torch.einsum("rhd,hdc->rhc", q2.double().reshape(q2.shape[0], wkh.shape[0], HD), wkh)


def logits(u_, xt):
    """scale * u[r,h,:] . x~[r,f,:]  (the original logits minus a term constant in f)"""
    return torch.einsum("rhc,rfc->rhf", u_.double(), xt.double()) * HD ** -0.5


def attn(logits_):
    return torch.softmax(logits_.double(), dim=-1)


def out(attn_, xt):
    R, heads, F = attn_.shape
    return torch.einsum("rhf,rfhd->rhd", attn_.double(), _xh(xt, heads)).reshape(R, heads * HD)


def da(dout, xt, heads):
    R = dout.shape[0]
    return torch.einsum("rhd,rfhd->rhf", dout.double().reshape(R, heads, HD), _xh(xt, heads))


def dl(attn_, dout, xt):
    a, d = attn_.double(), da(dout, xt, attn_.shape[1])
    return HD ** -0.5 * a * (d - (a * d).sum(-1, keepdim=True))


def g(dl_, xt):
    return torch.einsum("rhf,rfc->hrc", dl_.double(), xt.double())


def dxt(attn_, dl_, dout, u_):
    R, heads, F = attn_.shape
    ad = torch.einsum("rhf,rhd->rfhd", attn_.double(), dout.double().reshape(R, heads, HD)).reshape(R, F, heads * HD)
    return ad + torch.einsum("rhf,rhc->rfc", dl_.double(), u_.double())


def dq2(g_, wk):
    heads, R, C = g_.shape
    return torch.einsum("hrc,hdc->rhd", g_.double(), _wkh(wk)).reshape(R, C)


def dwk(q2, g_):
    heads, R, C = g_.shape
    return torch.einsum("rhd,hrc->hdc", q2.double().reshape(R, heads, HD), g_.double()).reshape(C, C)


# ---------------------------------------------------------------------------------------------------------------------
# magnitudes
# ---------------------------------------------------------------------------------------------------------------------
def mag_attn(a, u_, xt):
    """A_f = a_f (Ebar_f + sum_f' a_f' Ebar_f'),  Ebar = scale sum_c |x~||u|"""
    ebar = torch.einsum("rhc,rfc->rhf", u_.double().abs(), xt.double().abs()) * HD ** -0.5
    return a * (ebar + (a * ebar).sum(-1, keepdim=True))


def mag_dl(a, dout, xt):
    d = da(dout, xt, a.shape[1]).abs()
    return HD ** -0.5 * a * (d + (a * d).sum(-1, keepdim=True))


def mag_p(a, A, dout, xt):
    """P: what an error of A in attn2 does to dl, to first order"""
    d = da(dout, xt, a.shape[1]).abs()
    return HD ** -0.5 * (A * (d + (a * d).sum(-1, keepdim=True)) + a * (A * d).sum(-1, keepdim=True))


def _adout(a, dout):
    R, heads, F = a.shape
    return torch.einsum("rhf,rhd->rfhd", a, dout.double().abs().reshape(R, heads, HD)).reshape(R, F, heads * HD)


def quantities(inp, got, ex):
    """The checked parts of a result: [(what, got, want, magnitude, limit)], |got - want| <= limit * magnitude per element.
    inp: q2 [R,C], xt [R,F,C], wk [C,C], dout [R,C], heads.  got: attn, out, dl (compact [R,h,F]), g, dxt -- of the device
    or of time_rounded.  ex: time_exact's dict.  The stage rows feed each stage reference what `got` holds upstream."""
    q2, xt, wk, dout = inp["q2"], inp["xt"], inp["wk"], inp["dout"]
    xa = xt.double().abs()
    u_ = u(q2, wk)
    ua = u_.abs()
    a_ex = attn(logits(u_, xt))
    A = mag_attn(a_ex, u_, xt)
    ga, gdl = got["attn"].double(), got["dl"].double()
    dl_ref, mdl = dl(ga, dout, xt), mag_dl(ga, dout, xt)
    rows = [("attn2 | logits, softmax", ga, a_ex, A, LIM_ATT),
            ("out | time2_out", got["out"], out(ga, xt), out(ga, xa), LIM_OUT),
            ("dl | time2_dlg", gdl, dl_ref, mdl, LIM_DL),
            ("g | time2_dlg", got["g"], g(dl_ref, xt), g(mdl, xa), LIM_G),
            ("dx~ | time2_dx", got["dxt"], dxt(ga, gdl, dout, u_),
             _adout(ga, dout) + torch.einsum("rhf,rhc->rfc", gdl.abs(), ua), LIM_DX)]
    a, mdl, edl = ex["attn"], mag_dl(ex["attn"], dout, xt), ex["dl"].abs()
    P = mag_p(a, A, dout, xt)
    own = _adout(a, dout) + torch.einsum("rhf,rhc->rfc", edl, ua)
    rows += [("out vs exact", got["out"], ex["out"], out(a, xa) + out(A, xa), LIM_E2E),
             ("g vs exact", got["g"], ex["g"], g(mdl + P, xa), LIM_E2E),
             ("dx~ vs exact", got["dxt"], ex["dxt"],
              _adout(A, dout) + torch.einsum("rhf,rhc->rfc", mdl + P + edl, ua) + own, LIM_E2E)]
    return [(w, gt, wt, m + TINY, lim) for w, gt, wt, m, lim in rows]


def gw_quantities(g_, q2, wk, got):
    """dq2 and dWk of one pass over g (got: dq2 [R,C], dwk [C,C]) against the stage functions."""
    want = dq2(g_, wk)
    chain = dq2(g_.double().abs(), wk.double().abs())
    return [("dq2 | time2_gw", got["dq2"], want, want.abs() + FP32_CHAIN / LIM_DQ2 * chain + TINY, LIM_DQ2),
            ("dWk | time2_gw", got["dwk"], dwk(q2, g_), dwk(q2.double().abs(), g_.double().abs()) + TINY, FP32_CHAIN)]


def ratio(got, want, mag):
    """max |got - want| / mag; inf if anything is not finite"""
    got = got.double()
    return float(((got - want.double()).abs() / mag).max()) if bool(torch.isfinite(got).all()) else float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# the rounding model and its wrong variants
# ---------------------------------------------------------------------------------------------------------------------
# what each mutant gets wrong, and the rows it applies to: (heads, F, R) -> bool
MUTANTS = {
    "u_head_from_neighbour": lambda h, F, R: h >= 2,          # compute_u_tile picks the wrong q fragment (h != hfirst)
    "chunk_slab_dropped": lambda h, F, R: True,               # one chunk's partial logits missing for the rows of one tile
    "frames_swapped_last_row": lambda h, F, R: True,          # two frames of one head of the last row
    "tail_row_unmasked": lambda h, F, R: R >= 2,              # the clamped copy of row R-1 written over row R-2
    "dl_without_dot": lambda h, F, R: True,                   # dl = scale a da for one head
    "g_from_next_head": lambda h, F, R: h >= 2,               # g of head h built from dl of head h+1
    "dx_without_adout": lambda h, F, R: True,                 # a dout missing in one chunk
    "dl_pad_nonzero": lambda h, F, R: h < MAXH,               # the padded dl columns hold 1, the padded U rows head 0's
    "dwk_last_tile_missing": lambda h, F, R: True,            # the last 32-row tile of one split left out of dWk
    "dq2_tile_from_previous": lambda h, F, R: R >= 64,        # rows 32..63 of dq2 are rows 0..31
}


def gw_rounded(g_, q2, wk, rounding=True, mutant=None):
    """dq2 rounded once, dWk in fp32 (modelled exactly)."""
    r = r16 if rounding else _same
    heads, R, C = g_.shape
    dq, dw = dq2(g_, wk), dwk(q2, g_)
    if mutant == "dq2_tile_from_previous":
        dq = dq.clone()
        dq[32:64] = dq[0:32]
    if mutant == "dwk_last_tile_missing":                     # split 0's last tile (any R: the last <= 32 rows it owns)
        tps = gw_route(R)["tiles_per_split"] if R % GW_TR == 0 and R >= GW_TR else 1
        hi = min(R, tps * GW_TR)
        lo = max(0, hi - GW_TR)
        dw = dw - dwk(q2[lo:hi], g_[:, lo:hi])
    return {"dq2": r(dq), "dwk": dw}


def time_rounded(q2, xt, wk, dout, heads, rounding=True, mutant=None):
    """The chain evaluated the way the kernels evaluate it (flat layouts), fp64 between the points where they round to bf16
    (the list in the module docstring).  -> dict: attn, out, dl (compact, the bf16 the dx kernels read), dl16 [R,F,16] as
    stored, g, dxt, dq2, dwk."""
    assert mutant is None or mutant in MUTANTS
    r = r16 if rounding else _same
    R, F, C = xt.shape
    scale, nt = HD ** -0.5, (R + TQ - 1) // TQ
    x = xt.double()
    u_ = r(u(q2, wk))                                                       # [R,h,C]
    if mutant == "u_head_from_neighbour":
        u_ = u_.clone()
        u_[:, 1] = u_[:, 0]
    part = torch.einsum("rhkc,rfkc->rhfk", u_.reshape(R, heads, heads, HD), x.reshape(R, F, heads, HD)) * scale
    if mutant == "chunk_slab_dropped":
        t = min(1, nt - 1)
        part[t * TQ:(t + 1) * TQ, :, :, 0] = 0.0
    a = attn(part.sum(-1))
    if mutant == "frames_swapped_last_row":
        a = a.clone()
        a[R - 1, 0, :2] = a[R - 1, 0, :2].flip(0)
    o = r(out(a, x))
    d = da(dout, x, heads)
    dl_ = scale * a * (d - (a * d).sum(-1, keepdim=True))
    if mutant == "dl_without_dot":
        dl_ = dl_.clone()
        dl_[:, 0] = scale * a[:, 0] * d[:, 0]
    dl_g = dl_
    if mutant == "g_from_next_head":
        dl_g = dl_.clone()
        dl_g[:, 0] = dl_[:, 1]
    g_ = r(g(dl_g, x))
    dlb = r(dl_)
    dl16 = torch.zeros(R, F, MAXH, dtype=torch.float64, device=x.device)
    dl16[:, :, :heads] = dlb.transpose(1, 2)
    dx = dxt(a, dlb, dout, u_)
    if mutant == "dl_pad_nonzero":
        dl16[:, :, heads:] = 1.0
        dx = dx + (MAXH - heads) * u_[:, 0][:, None, :]
    if mutant == "dx_without_adout":
        dx[:, :, :HD] -= torch.einsum("rf,rd->rfd", a[:, 0], dout.double()[:, :HD])
    dx = r(dx)
    if mutant == "tail_row_unmasked":
        o, dx, g_, dlb, dl16, a = (t.clone() for t in (o, dx, g_, dlb, dl16, a))
        o[R - 2], dx[R - 2], dlb[R - 2], dl16[R - 2], a[R - 2] = o[R - 1], dx[R - 1], dlb[R - 1], dl16[R - 1], a[R - 1]
        g_[:, R - 2] = g_[:, R - 1]
    res = {"attn": a, "out": o, "dl": dlb, "dl16": dl16, "g": g_, "dxt": dx}
    res.update(gw_rounded(g_, q2, wk, rounding, mutant))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch restated
# ---------------------------------------------------------------------------------------------------------------------
def upw_of(heads):
    return (2 * heads + 7) // 8


def lds_staged_fwd(heads, F):
    """time2_lds_staged: 2 U buffers + 2 stages of (q2 tile, x~ tile)"""
    urow, qp, xp = heads * (HD * 2 + 16) + 16, heads * HD * 2 + 16, HD * 2 + 16
    return 2 * TQ * urow + 2 * TQ * qp + 2 * TQ * F * xp


def lds_staged_bwd(heads):
    return 2 * TQ * MAXH * (HD * 2 + 8) + 2 * TQ * (heads * HD * 2 + 16)


def instances(heads, F, lds=True):
    """(forward instance, ring depth), (backward instance, ring depth) of focus_traj_time2_fwd / _bwd"""
    w = upw_of(heads)
    fs = lds and F <= 8 and lds_staged_fwd(heads, F) <= LDS_MAX
    bs = lds and lds_staged_bwd(heads) <= LDS_MAX and not (w == 4 and F != 8)
    fwd = ("time2_logits_lds_kernel<%d,%d>" if fs else "time2_logits_kernel<%d,%d>") % (F, w), 2 if fs else 3
    bwd = ("time2_dx_lds_kernel<%d,%d>" if bs else "time2_dx_kernel<%d,%d>") % (F, w), 2 if bs else (2 if F > 8 else 3)
    return fwd, bwd


def owners(nchunk, spread=False, grid=GRID):
    """owner_of_block for every workgroup id: ([(cc, range) or None], nranges)"""
    table = []
    if spread:
        nranges = grid // nchunk
        for i in range(grid):
            table.append((i % nchunk, i // nchunk) if i < nranges * nchunk else None)
        return table, nranges
    gdiv = 1
    for dv in range(2, 9):
        if nchunk % dv == 0:
            gdiv = dv
    per_xcd = grid >> 3
    gpx, parts = per_xcd // gdiv, nchunk // gdiv
    nranges = 8 * gpx // parts
    for i in range(grid):
        xcd, j = i & 7, i >> 3
        gi = xcd + 8 * (j // gdiv)
        ok = j < gpx * gdiv and gi < nranges * parts
        table.append(((gi % parts) * gdiv + j % gdiv, gi // parts) if ok else None)
    return table, nranges


def turn_begin(ntiles, rng, nranges, depth):
    turns = (ntiles + depth - 1) // depth
    return (turns * rng // nranges) * depth


def route(case, lds=True, spread=False):
    """What the two launches of a row reach: instance, ring depth, nranges, ranges that own no tile, tiles run past
    ntiles (by the last non-empty range)."""
    _, B, S, F, heads = case[:5]
    rows = B * S
    ntiles = (rows + TQ - 1) // TQ
    _, nranges = owners(heads, spread)
    res = {"rows": rows, "ntiles": ntiles, "nranges": nranges}
    for key, (inst, depth) in zip(("fwd", "bwd"), instances(heads, F, lds)):
        spans = [(turn_begin(ntiles, r, nranges, depth), turn_begin(ntiles, r + 1, nranges, depth)) for r in range(nranges)]
        res[key] = {"instance": inst, "depth": depth, "empty": sum(1 for b, e in spans if e == b),
                    "past": spans[-1][1] - ntiles, "most_turns": max(e - b for b, e in spans) // depth}
    return res


def reachable_instances(lds=True):
    s = set()
    for F in (4, 8, 16):
        for heads in range(1, MAXH + 1):
            fwd, bwd = instances(heads, F, lds)
            s |= {fwd[0], bwd[0]}
    return s


def gw_route(R, heads=GW_HEADS):
    """gw_splits and the grid of focus_traj_time2_gw"""
    tiles = R // GW_TR
    splits = max(1, min(tiles, 256 // max(heads, 1)))
    tps = (tiles + splits - 1) // splits
    used = (tiles + tps - 1) // tps
    return {"tiles": tiles, "splits": splits, "tiles_per_split": tps, "used": used, "last": tiles - (used - 1) * tps}


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
# (id, B, S, F, heads, ldw, extra batch stride of out / dout in elements, flavour).  ldw: "C", "C+8" or "2C".
# flavours: unit -- logits of order 1; peaked -- every third row near one-hot; big -- logits of order +-60.
CASES = [
    # F = 4: staged logits for every head count; dx staged up to 12 heads, direct above
    ("f4_h1_r1", 1, 1, 4, 1, "2C", 0, "unit"),
    ("f4_h3_r15", 3, 5, 4, 3, "C", 24, "unit"),
    ("f4_h5_r17", 1, 17, 4, 5, "C+8", 0, "peaked"),
    ("f4_h9_s37", 3, 37, 4, 9, "2C", 8, "unit"),
    ("f4_h13_s21", 2, 21, 4, 13, "C", 0, "unit"),
    ("f4_h16_s50", 1, 50, 4, 16, "C+8", 0, "big"),
    # F = 8: staged logits up to 14 heads, direct for 15 and 16; dx staged throughout
    ("f8_h1_r16", 1, 16, 8, 1, "C", 0, "unit"),
    ("f8_h1_s35", 2, 35, 8, 1, "2C", 16, "peaked"),
    ("f8_h4_s19", 3, 19, 8, 4, "2C", 0, "unit"),
    ("f8_h8_s43", 2, 43, 8, 8, "C+8", 0, "unit"),
    ("f8_h11_s29", 1, 29, 8, 11, "2C", 0, "big"),
    ("f8_h12_r1280", 2, 640, 8, 12, "2C", 0, "unit"),       # 2 x (20 ranges x ring depth 2 x 16): whole turns, two each
    ("f8_h12_r1281", 3, 427, 8, 12, "2C", 0, "peaked"),     # the same plus one row
    ("f8_h13_s23", 2, 23, 8, 13, "C", 0, "unit"),
    ("f8_h14_s18", 1, 18, 8, 14, "2C", 0, "unit"),          # the last staged logits shape
    ("f8_h15_s33", 2, 33, 8, 15, "2C", 8, "unit"),          # the first direct one
    ("f8_h16_s300", 1, 300, 8, 16, "C", 0, "unit"),         # 19 tiles over 16 ranges: rings of 3 (logits) and 2 (dx)
    # F = 16: direct logits; dx staged up to 12 heads, direct above
    ("f16_h3_s21", 2, 21, 16, 3, "2C", 0, "unit"),
    ("f16_h5_r15", 1, 15, 16, 5, "C+8", 0, "unit"),
    ("f16_h8_s27", 3, 27, 16, 8, "C", 40, "peaked"),
    ("f16_h9_s33", 1, 33, 16, 9, "2C", 0, "unit"),
    ("f16_h12_s45", 2, 45, 16, 12, "2C", 0, "unit"),
    ("f16_h16_s21", 2, 21, 16, 16, "2C", 0, "unit"),
]

# (id, R, wk_ld): 12 heads, C = 768
GW_CASES = [("gw_r32", 32, 768), ("gw_r64", 64, 776), ("gw_r672", 672, 768), ("gw_r704", 704, 776), ("gw_r736", 736, 768),
            ("gw_r1376", 1376, 776)]


def ldw_of(case):
    C = case[4] * HD
    return {"C": C, "C+8": C + 8, "2C": 2 * C}[case[5]]


def bstride_of(case):
    """batch stride of out / dout in elements: the [1+S, C] rows of a batch plus the row's extra"""
    return (case[2] + 1) * case[4] * HD + case[6]


def inputs(case):
    """(q2 [B,S,C], x~ [B,S,F,C], Wk [C,C], bk [C], cls [B,1,C], ct [B,1+S,C]) of a row: bf16 on the CPU (bk fp64), seeded
    from the row's id.  unit: randn with Wk ~ C^-1/2, logits of order 1.  peaked: every third query (flat row % 3 == 0) is
    12 times the unit vector along Wk[h] x~ of frame (row % F), whose logit is then ~12 above the others.  big: q2 x 60."""
    name, B, S, F, heads = case[:5]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    C, R = heads * HD, B * S
    q2 = torch.randn(B, S, C, generator=gen)
    xt = torch.randn(B, S, F, C, generator=gen).bfloat16()
    wk = (torch.randn(C, C, generator=gen) * C ** -0.5).bfloat16()
    bk = torch.randn(C, generator=gen).double()
    cls = torch.randn(B, 1, C, generator=gen).bfloat16()
    ct = torch.randn(B, 1 + S, C, generator=gen).bfloat16()
    if case[7] == "peaked":
        rows = torch.arange(0, R, 3)
        k2 = (xt.reshape(R, F, C)[rows, rows % F].double() @ wk.double().t()).reshape(-1, heads, HD)
        qf = q2.reshape(R, heads, HD)
        qf[rows] = (12.0 * 8.0 * k2 / (k2 * k2).sum(-1, keepdim=True)).float()   # scale q . k2 = 12
        q2 = qf.reshape(B, S, C)
    elif case[7] == "big":
        q2 = q2 * 60.0
    else:
        assert case[7] == "unit"
    return q2.bfloat16(), xt, wk, bk, cls, ct


def flat(case, q2, xt, wk, ct):
    """The flat-layout dict `quantities` and time_rounded take."""
    _, B, S, F, heads = case[:5]
    C = heads * HD
    return {"q2": q2.reshape(B * S, C), "xt": xt.reshape(B * S, F, C), "wk": wk, "dout": ct[:, 1:].reshape(B * S, C),
            "heads": heads}


def gw_inputs(case):
    """(g [12,R,768], q2 [R,768], Wk [768,768]) bf16 on the CPU, seeded from the row's id."""
    name, R, _ = case
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return (torch.randn(GW_HEADS, R, GW_C, generator=gen).bfloat16(), torch.randn(R, GW_C, generator=gen).bfloat16(),
            (torch.randn(GW_C, GW_C, generator=gen) * GW_C ** -0.5).bfloat16())
