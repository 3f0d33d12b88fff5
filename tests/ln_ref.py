"""LayerNorm in fp64, the bounds its fp32 kernels have to keep, the route each shape takes, and the case table.

No GPU code and no import of focus_amd: tests/test_ln_ref_cpu.py checks this file on the CPU (the reference against
torch.nn.functional.layer_norm, an fp32 twin of each kernel family against the bounds, every mutant outside them, the
routes the table reaches); tests/test_gpu_layernorm.py runs the kernels of csrc/layernorm.hip against it.

Bounds (u = 2^-24, the fp32 unit roundoff; first order in u unless said otherwise).  Inputs are exact: the tests round
x, dy, dres to the storage type first, gamma and beta are fp32, eps is the fp32 value that crosses the ABI.

forward, per row (S1 = sum |x|, mu and var the exact mean and biased variance of the row):
  mean   a sum of D terms in any order is off by <= (D - 1) u S1; the division by D is one rounding, or (sub-wave
         kernels) a product with the rounded constant 1.f / D: two.  |d_mean| <= (D + 2) u S1 / D =: dm.
  var    q = sum (x - m)^2 with the computed mean m = mu + d: sum (x - m)^2 = sum (x - mu)^2 + D d^2 exactly (the cross
         term is 2 d sum(x - mu) = 0), so the mean's error enters at second order only -- but d^2 / var is not small
         against u where |mu| >> std (rows of mean 30, std 0.1), so it is kept: |d_var| <= (D + 3) u var + dm^2
         ((x - m): u, its square: u, the sum of D terms: (D - 1) u, the division: u or 2u -> D + 3).
  rstd   v = var + eps adds one rounding: rel(v) = ((D + 3) u var + dm^2) / (var + eps) + u.  (1 + e)^(-1/2) moves by
         e / 2 (1 + e) at most for e < 1/2; the hardware reciprocal square root is good to 2 ulp = 4u, and the
         result is stored after one more rounding: rel(rstd) = rel(v) (1 + rel(v)) / 2 + 5u.
  y      y = (x - m) rstd gamma + beta: |gamma| rstd (dm + u |x - mu|) for the subtraction, |y - beta| (rel(rstd) + 3u)
         for rstd and the two products, u |y| for the last sum.  A bf16 y is rounded to nearest once more:
         2^-8 (|y| + the bound so far).
backward, per row, from the fp32 mean and rstd it is given (so x^ = (x - mean) rstd is off by 2u relative),
  gd = dy gamma (u), G1 = sum |gd| / D, G2 = sum |gd x^| / D, m1 = sum gd / D, m2 = sum gd x^ / D:
  |d_m1| <= (D + 3) u G1          (products u, sum (D - 1) u, division <= 2u, one spare)
  |d_m2| <= (D + 5) u G2          (gd: u, x^: 2u, product: u, sum (D - 1) u, division <= 2u)
  dx = rstd (gd - m1 - x^ m2) + dres:
        rstd [u |gd| + d_m1 + |x^| d_m2 + 3u |x^ m2| + 2u (|gd| + |m1| + |x^ m2|)] + u |dx - dres| + u |dx|
        (x^ and the product x^ m2: 3u; the two subtractions: u each of at most |gd| + |m1| + |x^ m2|; the product with
        rstd; the sum with dres).  bf16: + 2^-8 (|dx| + that).
  dgamma, dbeta, column sums of `partial`: a term dy x^ is off by 3u, a sum of `rows` terms through nblk block partials
        and the 16 lanes of the finish kernel by at most (rows + nblk + 16) u sum |terms| in any order.
  column sums of `partial` (fp64) against the dgamma / dbeta the finish kernel makes of them: (nblk + 16) u sum |partial|.
Every element is checked against its own bound; nothing is excluded."""
import math
import zlib

import torch

U = 2.0 ** -24
BF = 2.0 ** -8
F64 = torch.float64


# ---- the reference ------------------------------------------------------------------------------------------------
def fwd(x, gamma, beta, eps):
    """-> y [rows, D], mean [rows], rstd [rows] in fp64."""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    mean = x.mean(-1)
    xc = x - mean[:, None]
    var = (xc * xc).mean(-1)
    rstd = 1.0 / torch.sqrt(var + float(eps))
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def bwd(dy, x, gamma, mean, rstd, dres=None):
    """-> dx, dgamma, dbeta in fp64 from the mean and rstd it is given."""
    dy, x, gamma, mean, rstd = dy.to(F64), x.to(F64), gamma.to(F64), mean.to(F64), rstd.to(F64)
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = dy * gamma
    m1, m2 = gd.mean(-1, keepdim=True), (gd * xh).mean(-1, keepdim=True)
    dx = rstd[:, None] * (gd - m1 - xh * m2)
    if dres is not None:
        dx = dx + dres.to(F64)
    return dx, (dy * xh).sum(0), dy.sum(0)


def row_offsets(rows, rpb, xbs, D, device=None):
    """Element offset of every row of a row-block tensor: block = row // rpb, offset = block * xbs + (row % rpb) * D."""
    r = torch.arange(rows, dtype=torch.int64, device=device)
    return (r // rpb) * xbs + (r % rpb) * D


def gather_rows(flat, base, rows, rpb, xbs, D):
    """[rows, D] read out of the flat buffer, element by element."""
    idx = base + row_offsets(rows, rpb, xbs, D, flat.device)[:, None] + torch.arange(D, device=flat.device)[None, :]
    return flat[idx]


def scatter_rows(flat, base, vals, rpb, xbs):
    rows, D = vals.shape
    idx = base + row_offsets(rows, rpb, xbs, D, flat.device)[:, None] + torch.arange(D, device=flat.device)[None, :]
    flat[idx] = vals
    return flat


# ---- the bounds ---------------------------------------------------------------------------------------------------
def fwd_bounds(x, gamma, beta, eps, bf16_out):
    """-> bounds of mean [rows], rstd [rows], y [rows, D] (absolute), from the exact inputs."""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    D = x.shape[-1]
    y, mean, rstd = fwd(x, gamma, beta, eps)
    xc = x - mean[:, None]
    var = (xc * xc).mean(-1)
    dm = (D + 2) * U * x.abs().sum(-1) / D
    relv = ((D + 3) * U * var + dm * dm) / (var + float(eps)) + U
    relr = 0.5 * relv * (1 + relv) + 5 * U
    by = gamma.abs() * rstd[:, None] * (dm[:, None] + U * xc.abs()) + (y - beta).abs() * (relr[:, None] + 3 * U) + U * y.abs()
    if bf16_out:
        by = by + BF * (y.abs() + by)
    return dm, relr * rstd, by


def bwd_bounds(dy, x, gamma, mean, rstd, dres, bf16_out):
    """-> absolute bound of dx [rows, D] from the exact inputs."""
    dy, x, gamma, mean, rstd = dy.to(F64), x.to(F64), gamma.to(F64), mean.to(F64), rstd.to(F64)
    D = x.shape[-1]
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = dy * gamma
    m1, m2 = gd.mean(-1, keepdim=True), (gd * xh).mean(-1, keepdim=True)
    G1, G2 = gd.abs().mean(-1, keepdim=True), (gd * xh).abs().mean(-1, keepdim=True)
    core = rstd[:, None] * (gd - m1 - xh * m2)
    xm = (xh * m2).abs()
    b = rstd[:, None] * (U * gd.abs() + (D + 3) * U * G1 + xh.abs() * (D + 5) * U * G2 + 3 * U * xm
                         + 2 * U * (gd.abs() + m1.abs() + xm)) + U * core.abs()
    full = core if dres is None else core + dres.to(F64)
    b = b + U * full.abs()
    if bf16_out:
        b = b + BF * (full.abs() + b)
    return b


def col_scale(dy, x, mean, rstd):
    """-> sum |dy x^|, sum |dy| per column: times (rows + nblk + 16) u they bound dgamma, dbeta and the sums of `partial`."""
    dy, x = dy.to(F64), x.to(F64)
    xh = (x - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]
    return (dy * xh).abs().sum(0), dy.abs().sum(0)


# ---- the route: a transcription of the dispatch of csrc/layernorm.hip ----------------------------------------------
def bwd_blocks(rows):
    """focus_layernorm_bwd_blocks."""
    return max(1, min(512, (rows + 3) // 4))


def route(rows, D, dtype, xbs, align_bytes, direction):
    """Which kernel a call takes.  Mirrors ln_v16_ok (rows >= 4096, bf16, D % 8 == 0, D <= 1024, xbs % 8 == 0, every row
    pointer 16-byte aligned), LN_V16_DISPATCH (LPR, NV by D), ln_fwd_launch / ln_bwd_launch (nv = (D + 255) / 256 rounded
    up to 1, 2, 3, 4, 8, 16), the LNF macro of ln_fwd_any (per_blk rows per block, the grid capped at 4096 blocks) and the
    LNB macro of ln_bwd_any (`wide`: 8 waves once rows >= nblk * 256).  align_bytes: the alignment of the least aligned
    of the row pointers of the call (x, y forward; dy, x, dx, dres backward); gamma and beta are 16-byte aligned.
    -> family ('wave' | 'sub'), LPR (sub), NV, NW, trips (forward grid-stride loop), nblk, pass_rows (rows one trip of the
    grid takes, the unit of the row loops), lds (dynamic LDS bytes, sub backward)."""
    assert direction in ("fwd", "bwd") and dtype in ("fp32", "bf16")
    nblk = bwd_blocks(rows)
    sub = rows >= 4096 and dtype == "bf16" and D % 8 == 0 and D <= 1024 and xbs % 8 == 0 and align_bytes % 16 == 0
    if sub:
        LPR, NV = (8, 1) if D <= 64 else (16, 1) if D <= 128 else (32, 1) if D <= 256 else (64, 1) if D <= 512 else (64, 2)
        RPW, UN = 64 // LPR, 4 if NV == 1 else 2
        if direction == "fwd":
            per_blk = 4 * RPW * UN
            grid = min((rows + per_blk - 1) // per_blk, 4096)
            return dict(family="sub", LPR=LPR, NV=NV, NW=4, trips=-(-rows // (grid * per_blk)), nblk=grid,
                        pass_rows=grid * per_blk, lds=0)
        NW = 8 if rows >= nblk * 4 * 64 else 4
        pr = nblk * NW * RPW * UN
        return dict(family="sub", LPR=LPR, NV=NV, NW=NW, trips=-(-rows // pr), nblk=nblk, pass_rows=pr,
                    lds=2 * NW * RPW * D * 4)
    nv = (D + 255) // 256
    NV = next(n for n in (1, 2, 3, 4, 8, 16) if nv <= n)
    if direction == "fwd":
        grid = (rows + 3) // 4
        return dict(family="wave", LPR=None, NV=NV, NW=4, trips=1, nblk=grid, pass_rows=grid * 4, lds=0)
    pr = 2 * nblk * 4                                     # two rows per iteration
    return dict(family="wave", LPR=None, NV=NV, NW=4, trips=-(-rows // pr), nblk=nblk, pass_rows=pr, lds=0)


def edge_rows(rows, pass_rows):
    """Row 0, the last row of the first pass, the first row of the second pass, the first row of the last pass, rows - 1."""
    e = {0, min(pass_rows, rows) - 1, rows - 1, ((rows - 1) // pass_rows) * pass_rows}
    if pass_rows < rows:
        e.add(pass_rows)
    return sorted(e)


# ---- the case table -----------------------------------------------------------------------------------------------
# A case: direction, dtype, rows, D; rpb / T / frame / pad: x (and dx) as rows // rpb blocks of rpb rows inside a
# [B, T, rpb, D (+ pad elements per block)] buffer, the pointer at frame `frame` (rpb None: dense); off: elements the base
# pointer of x (and dx) is moved off its 16-byte alignment; xcls: 'randn' (randn * 2 + 0.5), 'tiny' (1e-3 randn: variance
# about eps), 'offset' (30 + 0.1 randn); eps; gcls: 'signed0' (randn, column 1 exactly zero) | 'ones'; dres; dycls: 'randn' |
# 'edge' (zero outside edge_rows()); group: the test the GPU file runs it in.
def _case(direction, dtype, rows, D, group, **kw):
    c = dict(dir=direction, dtype=dtype, rows=rows, D=D, group=group, rpb=None, T=1, frame=0, pad=0, off=0, xcls="randn",
             eps=1e-6, gcls="signed0", dres=False, dycls="randn")
    c.update(kw)
    if c["rpb"] is not None:
        assert rows % c["rpb"] == 0
    return c


def case_id(c):
    s = "%s-%s-%dx%d" % (c["dir"], c["dtype"], c["rows"], c["D"])
    if c["rpb"] is not None:
        s += "-rpb%d-T%d-f%d" % (c["rpb"], c["T"], c["frame"])
    if c["pad"]:
        s += "-pad%d" % c["pad"]
    if c["off"]:
        s += "-off%d" % c["off"]
    if c["xcls"] != "randn":
        s += "-%s-eps%g" % (c["xcls"], c["eps"])
    if c["gcls"] != "signed0":
        s += "-g" + c["gcls"]
    if c["dres"]:
        s += "-dres"
    if c["dycls"] != "randn":
        s += "-" + c["dycls"]
    return s


def xbs_of(c):
    return 0 if c["rpb"] is None else c["T"] * c["rpb"] * c["D"] + c["pad"]


def rpb_of(c):
    return c["rows"] if c["rpb"] is None else c["rpb"]


def align_of(c):
    return 16 if c["off"] % (4 if c["dtype"] == "fp32" else 8) == 0 else 8


def route_of(c):
    return route(c["rows"], c["D"], c["dtype"], xbs_of(c), align_of(c), c["dir"])


WAVE_D = (4, 12, 252, 256, 260, 768, 772, 1024, 1028, 2048, 2052, 4096)       # first and last D of NV = 1, 2, 3, 4, 8, 16
WAVE_ROWS = (1, 3, 4, 5, 9)
SUB_D = ((8, 64), (72, 128), (136, 256), (264, 512), (520, 1024))              # smallest and largest D of each (LPR, NV)
_XCLS = (("randn", 1e-6), ("tiny", 1e-5), ("offset", 1e-6), ("tiny", 1e-6), ("randn", 1e-5))


def _build():
    cs = []
    for direction in ("fwd", "bwd"):
        # wave per row: rows around the 4 of a block, the first and last D of every NV
        for dtype in ("fp32", "bf16"):
            for i, D in enumerate(WAVE_D):
                for j, rows in enumerate(WAVE_ROWS):
                    xcls, eps = _XCLS[(i + j) % len(_XCLS)]
                    cs.append(_case(direction, dtype, rows, D, "wave-%s-%s-D%d" % (direction, dtype, D), xcls=xcls, eps=eps,
                                    dres=direction == "bwd" and rows in (3, 9), gcls="ones" if (i + j) % 4 == 3 else "signed0"))
        # bf16 with >= 4096 rows that still is wave per row: D % 8 == 4, D > 1024, a base 8 but not 16 bytes aligned, xbs % 8 == 4
        g = "wave-%s-bf16-4100" % direction
        cs.append(_case(direction, "bf16", 4100, 196, g))
        cs.append(_case(direction, "bf16", 4100, 1032, g, dres=direction == "bwd"))
        cs.append(_case(direction, "bf16", 4100, 192, g, off=4))
        cs.append(_case(direction, "bf16", 4100, 192, g, rpb=1025, T=3, frame=1, pad=4))
        # a sub-wave per row: every (LPR, NV) at its smallest and largest D, rows around a ragged last pass
        for lo_hi in SUB_D:
            for D in lo_hi:
                r = route(4096, D, "bf16", 0, 16, direction)
                step = (64 // r["LPR"]) * (4 if r["NV"] == 1 else 2)
                for rows in (4096, 4097, 4096 + step - 1, 4096 + step + 1):
                    cs.append(_case(direction, "bf16", rows, D, "sub-%s-D%d" % (direction, D), dres=direction == "bwd" and rows == 4097,
                                    xcls="tiny" if rows == 4096 + step + 1 else "randn", eps=1e-5))
        # row blocks, both families: rpb that no pass divides; T = 3 with the pointer at each frame, and adjacent blocks
        for dtype, rpb, B, D in (("fp32", 7, 3, 12), ("bf16", 7, 3, 260), ("fp32", 1025, 3, 196), ("bf16", 1025, 3, 196),
                                 ("bf16", 2051, 2, 192), ("bf16", 2051, 3, 520)):
            g = "blocks-%s-%s-%dx%dx%d" % (direction, dtype, B, rpb, D)
            for frame in (0, 1, 2):
                cs.append(_case(direction, dtype, B * rpb, D, g, rpb=rpb, T=3, frame=frame))
            cs.append(_case(direction, dtype, B * rpb, D, g, rpb=rpb, T=1))
    # inputs whose variance is about eps, and a mean 300 times the deviation, at one small shape in both types
    for dtype in ("fp32", "bf16"):
        for xcls, eps in (("tiny", 1e-5), ("tiny", 1e-6), ("offset", 1e-6)):
            cs.append(_case("fwd", dtype, 5, 256, "cond-fwd-" + dtype, xcls=xcls, eps=eps))
    # backward, the row loop more than once (nblk = 512)
    for dtype, rows in (("fp32", 2049), ("bf16", 2049), ("fp32", 4100)):
        for D in (12, 772):
            cs.append(_case("bwd", dtype, rows, D, "wave-bwd-%s-%d" % (dtype, rows), dres=D == 12))
    # forward, the second trip of the grid-stride loop: 4096 * per_blk + 3 rows at the smallest D of each (LPR, NV)
    for (D, _), per_blk in zip(SUB_D, (128, 64, 32, 16, 8)):
        cs.append(_case("fwd", "bf16", 4096 * per_blk + 3, D, "trip2-fwd-D%d" % D))
    # backward, 8-wave workgroups, with and without dres (D = 1024: 64 KiB of LDS)
    for _, D in SUB_D:
        for dres in (False, True):
            cs.append(_case("bwd", "bf16", 131072 + 5, D, "wide-bwd-D%d" % D, dres=dres))
    # edge-row probes: dy is zero outside edge_rows(); one per family and NW
    cs.append(_case("bwd", "fp32", 8200, 12, "edge", dycls="edge"))
    cs.append(_case("bwd", "bf16", 8200, 260, "edge", dycls="edge"))
    cs.append(_case("bwd", "bf16", 4100, 520, "edge", dycls="edge"))
    cs.append(_case("bwd", "bf16", 131072 + 5, 64, "edge", dycls="edge"))
    cs.append(_case("bwd", "fp32", 9, 12, "edge", dycls="edge"))
    seen, out = set(), []
    for c in cs:                                         # (4096 + step - 1 is 4097 where a pass takes 2 rows)
        if case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)
    return out


CASES = _build()
GROUPS = sorted({c["group"] for c in CASES})


def group(name):
    return [c for c in CASES if c["group"] == name]


def torch_dtype(c):
    return torch.float32 if c["dtype"] == "fp32" else torch.bfloat16


def inputs(c, device="cpu"):
    """-> dict of the case's tensors, x / dy / dres rounded to the storage type: x [rows, D] (the values of the rows; the test
    lays them out), gamma, beta (fp32), eps (the fp32 value as a Python float), dy, dres (backward)."""
    g = torch.Generator(device=device).manual_seed(zlib.crc32(case_id(c).encode()))
    rows, D, dt = c["rows"], c["D"], torch_dtype(c)
    rn = lambda *s: torch.randn(*s, generator=g, device=device, dtype=torch.float32)
    x = rn(rows, D)
    x = {"randn": lambda: x * 2 + 0.5, "tiny": lambda: x * 1e-3, "offset": lambda: x * 0.1 + 30.0}[c["xcls"]]()
    out = dict(x=x.to(dt))
    if c["gcls"] == "signed0":
        gamma = rn(D)
        gamma[1] = 0.0
    else:
        gamma = torch.ones(D, device=device)
    out.update(gamma=gamma, beta=rn(D), eps=float(torch.tensor(c["eps"], dtype=torch.float32)))
    if c["dir"] == "bwd":
        dy = rn(rows, D)
        if c["dycls"] == "edge":
            keep = torch.zeros(rows, 1, device=device)
            keep[edge_rows(rows, route_of(c)["pass_rows"])] = 1.0
            dy = dy * keep
        out["dy"] = dy.to(dt)
        out["dres"] = rn(rows, D).to(dt) if c["dres"] else None
    return out


def chunked(fn, kinds, rows, *tensors, chunk=16384):
    """fn over row chunks of the [rows, ...] tensors (None passes through).  fn returns a tuple; kinds has one letter per
    entry: 'r' row-wise (the chunks are concatenated) or 'c' a column sum (the chunks are added)."""
    parts = [fn(*[None if t is None else t[a:a + chunk] for t in tensors]) for a in range(0, rows, chunk)]
    return tuple(torch.cat([p[k] for p in parts]) if kind == "r" else sum(p[k] for p in parts) for k, kind in enumerate(kinds))


# ---- fp32 twins of the two kernel families (CPU; torch float32, one rounding per operation, no fused multiply-add) --
def _butterfly(s):
    """xor-shuffle reduction over the last axis (a power of two): what wave_sum / sub_sum compute, in their order."""
    n = s.shape[-1]
    idx = torch.arange(n)
    o = n // 2
    while o > 0:
        s = s + s[..., idx ^ o]
        o //= 2
    return s[..., 0]


def _lanes(t, r):
    """[rows, D] -> [rows, NV, lanes, per] zero padded, and the mask of real columns."""
    rows, D = t.shape
    lanes, per = (64, 4) if r["family"] == "wave" else (r["LPR"], 8)
    # the compiled NV may exceed what D needs; the extra vectors are inactive
    nv = -(-D // (lanes * per))
    pad = nv * lanes * per
    out = torch.zeros(rows, pad, dtype=torch.float32)
    out[:, :D] = t.float()
    mask = (torch.arange(pad) < D).view(1, nv, lanes, per)
    return out.view(rows, nv, lanes, per), mask


def _lane_sum(v, r):
    """Per-lane sum over the vectors in the kernel's order, then the butterfly -> [rows]."""
    s = torch.zeros(v.shape[0], v.shape[2], dtype=torch.float32)
    for i in range(v.shape[1]):
        if r["family"] == "wave":
            s = s + (((v[:, i, :, 0] + v[:, i, :, 1]) + v[:, i, :, 2]) + v[:, i, :, 3])
        else:
            for e in range(8):
                s = s + v[:, i, :, e]
    return _butterfly(s)


def _div(s, D, r):
    f32 = torch.float32
    return s / torch.tensor(float(D), dtype=f32) if r["family"] == "wave" else s * (torch.tensor(1.0, dtype=f32) / torch.tensor(float(D), dtype=f32))


def twin_fwd(x, gamma, beta, eps, r):
    rows, D = x.shape
    v, mask = _lanes(x, r)
    mu = _div(_lane_sum(v, r), D, r)
    a = torch.where(mask, v - mu.view(-1, 1, 1, 1), torch.zeros((), dtype=torch.float32))
    rs = 1.0 / torch.sqrt(_div(_lane_sum(a * a, r), D, r) + torch.tensor(eps, dtype=torch.float32))
    xc = a.reshape(rows, -1)[:, :D]
    y = xc * rs[:, None] * gamma.float() + beta.float()
    return y.to(x.dtype), mu, rs


def _accumulate(terms, r, rows):
    """Column sums of terms [rows, D] in the order of the kernels: per wave (or sub-wave) over the rows it visits, across
    the block's waves, then ln_bwd_finish (16 row-lanes striding the blocks, then their sum) -> partial [nblk, D], sum [D]."""
    nblk, D = r["nblk"], terms.shape[1]
    row = torch.arange(rows)
    if r["family"] == "wave":
        stride = nblk * 4
        acc, step, per_blk = row % stride, row // stride, 4
    else:
        RPW, UN = 64 // r["LPR"], 4 if r["NV"] == 1 else 2
        chunk, nwaves = RPW * UN, nblk * r["NW"]
        c, within = row // chunk, row % chunk
        acc, step, per_blk = (c % nwaves) * RPW + within % RPW, (c // nwaves) * UN + within // RPW, r["NW"] * RPW
    sums = torch.zeros(nblk * per_blk, D, dtype=torch.float32)
    for s in range(int(step.max()) + 1):
        sel = step == s
        sums[acc[sel]] = sums[acc[sel]] + terms[sel]
    sums = sums.view(nblk, per_blk, D)
    partial = sums[:, 0].clone()
    for k in range(1, per_blk):
        partial = partial + sums[:, k]
    K = -(-nblk // 16)
    padded = torch.zeros(K * 16, D, dtype=torch.float32)
    padded[:nblk] = partial
    padded = padded.view(K, 16, D)
    a = torch.zeros(16, D, dtype=torch.float32)
    for k in range(K):
        a = a + padded[k]
    t = torch.zeros(D, dtype=torch.float32)
    for k in range(16):
        t = t + a[k]
    return partial, t


def twin_bwd(dy, x, gamma, mean, rstd, dres, r):
    rows, D = x.shape
    mu, rs = mean.float()[:, None], rstd.float()[:, None]
    xh = (x.float() - mu) * rs
    gd = dy.float() * gamma.float()
    vg, _ = _lanes(gd, r)
    vx, _ = _lanes(gd * xh, r)
    m1, m2 = _div(_lane_sum(vg, r), D, r)[:, None], _div(_lane_sum(vx, r), D, r)[:, None]
    dx = rs * (gd - m1 - xh * m2)
    if dres is not None:
        dx = dx + dres.float()
    pg, dg = _accumulate(dy.float() * xh, r, rows)
    pb, db = _accumulate(dy.float(), r, rows)
    return dx.to(x.dtype), dg, db, torch.stack([pg, pb])


# ---- mutants: named wrong versions of the operation, in fp64 unless said otherwise ----------------------------------
def _is(c, **kw):
    return all(c[k] == v for k, v in kw.items())


def m_var_dm1(c, t):
    x = t["x"].to(F64)
    D = x.shape[1]
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).sum(-1) / max(D - 1, 1) + t["eps"])
    return dict(y=xc * rstd[:, None] * t["gamma"].to(F64) + t["beta"].to(F64), mean=mean, rstd=rstd)


def m_eps_outside(c, t):
    x = t["x"].to(F64)
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / (torch.sqrt((xc * xc).mean(-1)) + t["eps"])
    return dict(y=xc * rstd[:, None] * t["gamma"].to(F64) + t["beta"].to(F64), mean=mean, rstd=rstd)


def m_one_pass_fp32(c, t):
    x = t["x"].float()
    mean = x.mean(-1)
    var = (x * x).mean(-1) - mean * mean
    rstd = 1.0 / torch.sqrt(var + torch.tensor(t["eps"], dtype=torch.float32))
    y = (x - mean[:, None]) * rstd[:, None] * t["gamma"] + t["beta"]
    return dict(y=y.to(F64), mean=mean.to(F64), rstd=rstd.to(F64))


def m_last_row_stale(c, t):
    y, mean, rstd = fwd(t["x"], t["gamma"], t["beta"], t["eps"])
    y[-1], mean[-1], rstd[-1] = y[-2], mean[-2], rstd[-2]
    return dict(y=y, mean=mean, rstd=rstd)


def m_div_mod_swapped(c, t):
    """The rows read at block = row % rpb, offset = block * xbs + (row // rpb) * D, clamped into the buffer."""
    rows, D, rpb, xbs = c["rows"], c["D"], rpb_of(c), xbs_of(c)
    B = rows // rpb
    flat = torch.zeros(B * xbs, dtype=F64)
    base = c["frame"] * rpb * D
    scatter_rows(flat, base, t["x"].to(F64), rpb, xbs)
    r = torch.arange(rows)
    off = ((r % rpb) * xbs + (r // rpb) * D + base) % (B * xbs - D)
    x = flat[off[:, None] + torch.arange(D)[None, :]]
    y, mean, rstd = fwd(x, t["gamma"], t["beta"], t["eps"])
    return dict(y=y, mean=mean, rstd=rstd)


def _bwd_parts(t):
    _, mean, rstd = fwd(t["x"], t["gamma"], t["beta"], t["eps"])
    mean, rstd = mean.float(), rstd.float()
    return mean, rstd


def m_dx_no_m2(c, t):
    mean, rstd = _bwd_parts(t)
    dy, x, g = t["dy"].to(F64), t["x"].to(F64), t["gamma"].to(F64)
    gd = dy * g
    dx = rstd.to(F64)[:, None] * (gd - gd.mean(-1, keepdim=True))
    if t["dres"] is not None:
        dx = dx + t["dres"].to(F64)
    return dict(dx=dx)


def m_dres_twice(c, t):
    mean, rstd = _bwd_parts(t)
    return dict(dx=bwd(t["dy"], t["x"], t["gamma"], mean, rstd, t["dres"])[0] + t["dres"].to(F64))


def m_dres_dropped(c, t):
    mean, rstd = _bwd_parts(t)
    return dict(dx=bwd(t["dy"], t["x"], t["gamma"], mean, rstd, None)[0])


def _dgamma_without(c, t, row):
    mean, rstd = _bwd_parts(t)
    keep = torch.ones(c["rows"], dtype=torch.bool)
    keep[row] = False
    _, dg, db = bwd(t["dy"][keep], t["x"][keep], t["gamma"], mean[keep], rstd[keep])
    return dict(dgamma=dg, dbeta=db)


def m_dgamma_no_last_row(c, t):
    return _dgamma_without(c, t, c["rows"] - 1)


def m_dgamma_no_first_of_last_pass(c, t):
    return _dgamma_without(c, t, ((c["rows"] - 1) // route_of(c)["pass_rows"]) * route_of(c)["pass_rows"])


_small = lambda c: c["rows"] <= 9 and c["rpb"] is None
MUTANTS = [   # name, the wrong operation, the cases it is tried on
    ("variance over D - 1", m_var_dm1, lambda c: c["dir"] == "fwd" and _small(c) and c["D"] <= 260),
    ("eps added after the square root", m_eps_outside, lambda c: c["dir"] == "fwd" and c["xcls"] == "tiny" and c["rows"] <= 9),
    ("one-pass variance in fp32", m_one_pass_fp32, lambda c: c["dir"] == "fwd" and c["xcls"] == "offset" and c["rows"] <= 9),
    ("last row computed from row rows - 2", m_last_row_stale, lambda c: c["dir"] == "fwd" and c["rows"] in (5, 9, 4097) and c["D"] <= 64),
    ("/ and % of the block addressing swapped", m_div_mod_swapped,
     lambda c: c["dir"] == "fwd" and c["rpb"] in (7, 1025) and c["pad"] == 0),
    ("dx without its m2 term", m_dx_no_m2, lambda c: c["dir"] == "bwd" and _small(c) and c["dycls"] == "randn" and c["D"] <= 260),
    ("dres added twice", m_dres_twice, lambda c: c["dir"] == "bwd" and c["dres"] and c["rows"] <= 4100 and c["D"] <= 260),
    ("dres not added", m_dres_dropped, lambda c: c["dir"] == "bwd" and c["dres"] and c["rows"] <= 4100 and c["D"] <= 260),
    ("dgamma without the last row", m_dgamma_no_last_row, lambda c: c["dycls"] == "edge" and c["rows"] <= 8200),
    ("dgamma without the first row of the last pass", m_dgamma_no_first_of_last_pass, lambda c: c["dycls"] == "edge" and c["rows"] <= 8200),
]


def worst_ratio(got, want, bound):
    """Largest |got - want| / bound; an element whose bound is 0 has to be exact.  NaN or Inf count as infinite."""
    e = (got.to(F64) - want).abs()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
    zero = bound == 0
    if bool((e[zero] != 0).any()):
        return math.inf
    if bool(zero.all()):
        return 0.0
    return float((e[~zero] / bound[~zero]).max())


def fwd_ratios(c, t, got):
    """got: y, mean, rstd (any float type) -> {name: largest error / bound} against fp64."""
    def f(x):
        y, mean, rstd = fwd(x, t["gamma"], t["beta"], t["eps"])
        bm, br, by = fwd_bounds(x, t["gamma"], t["beta"], t["eps"], c["dtype"] == "bf16")
        return y, mean, rstd, bm, br, by
    y, mean, rstd, bm, br, by = chunked(f, "rrrrrr", c["rows"], t["x"])
    return dict(y=worst_ratio(got["y"], y, by), mean=worst_ratio(got["mean"], mean, bm), rstd=worst_ratio(got["rstd"], rstd, br))


def ref_stats(t, rows):
    """The reference's mean and rstd rounded to fp32: what the backward kernels are given."""
    mean, rstd = chunked(lambda x: fwd(x, t["gamma"], t["beta"], t["eps"])[1:], "rr", rows, t["x"])
    return mean.float(), rstd.float()


def bwd_ratios(c, t, mean, rstd, got):
    """got: any of dx, dgamma, dbeta, partial [2, nblk, D] -> {name: largest error / bound}."""
    nblk = bwd_blocks(c["rows"])
    bf = c["dtype"] == "bf16"

    def f(dy, x, mu, rs, dres):
        dx, dg, db = bwd(dy, x, t["gamma"], mu, rs, dres)
        sg, sb = col_scale(dy, x, mu, rs)
        return dx, bwd_bounds(dy, x, t["gamma"], mu, rs, dres, bf), dg, db, sg, sb
    dx, bdx, dg, db, sg, sb = chunked(f, "rrcccc", c["rows"], t["dy"], t["x"], mean, rstd, t["dres"])
    bg, bb = (c["rows"] + nblk + 16) * U * sg, (c["rows"] + nblk + 16) * U * sb
    out = {}
    if "dx" in got:
        out["dx"] = worst_ratio(got["dx"], dx, bdx)
    if "dgamma" in got:
        out["dgamma"] = worst_ratio(got["dgamma"], dg, bg)
        out["dbeta"] = worst_ratio(got["dbeta"], db, bb)
    if "partial" in got:
        p = got["partial"].to(F64)
        out["sum partial[0]"] = worst_ratio(p[0].sum(0), dg, bg)
        out["sum partial[1]"] = worst_ratio(p[1].sum(0), db, bb)
        if "dgamma" in got:
            k = (nblk + 16) * U
            out["finish dgamma"] = worst_ratio(got["dgamma"], p[0].sum(0), k * p[0].abs().sum(0))
            out["finish dbeta"] = worst_ratio(got["dbeta"], p[1].sum(0), k * p[1].abs().sum(0))
    return out
