"""Pooling attention in token layout in fp64 (csrc/token_pool.hip), the bounds its fp32 kernels have to keep, the walk of their
grids, the case table and mutants.

No GPU code and no import of focus_amd: tests/test_token_pool_ref_cpu.py checks this file on the CPU (the formulas against
F.conv3d / F.max_pool3d / F.avg_pool3d + F.layer_norm through the permutes of attention_pool, values and all gradients; an fp32
twin of every stage inside the bounds; every mutant outside them); tests/test_gpu_token_pool.py runs the kernels against it.

Layout.  x is [B, cls + T*H*W, C] rows, the columns are C / head_dim heads of head_dim; the row of cell (t, h, w) is
cls + (t*H + h)*W + w; with cls row 0 passes unpooled.  Output extents o = (i + 2p - k) // s + 1.  tap = (kt*KH + kh)*KW + kw.

Bounds (u = 2^-24, first order in u unless said otherwise).  Inputs are exact: the tests round x and the gradients to the
storage type first; weights and norm parameters are fp32.  A bf16 result is rounded to nearest once more: bf_round(), half a
unit in the last place of the value plus its bound (exact); an fp32 result is the accumulator itself.
  conv, avg   K = kt*kh*kw products accumulated in fp32 in a fixed order (fused or not: at most one rounding per product and
              one per addition, a division by K for avg): (K + 1) u sum |w x| per element, w = 1 / K for avg.
  max         values and indices are exact.  The cls row is a copy: exact.
  LayerNorm   the kernel normalises the UN-ROUNDED fp32 pooled values p~ = p + d, |d| <= e the bound above (no storage
              rounding).  tests/ln_ref.py bounds the fp32 LayerNorm of exact inputs; the perturbation d moves the exact result
              by the Jacobian: d_mean = mean(d), d_rstd = -rstd^2 mean(x^ d), d_y_j = gamma_j rstd (d_j - mean(d) - x^_j mean(x^ d)),
              so |d_mean| <= mean(e), |d_rstd| <= rstd^2 mean(|x^| e), |d_y_j| <= |gamma_j| rstd (e_j + mean(e) + |x^_j| mean(|x^| e)).
              The remainder is second order in rstd * e, which is below 2^-18 here (e <= 28 u sum |w x|): it is covered by
              charging the first-order terms 1 + 2^-10 times.
  dx          a gather of at most K terms: (K + 1) u sum |w dpooled| (max: the terms whose index matches; avg: w = 1 / K)
              [+ bf_round].  The cls row is a copy of dpooled row 0: exact.
  dw          n = B * heads * ot*oh*ow terms per element through row lanes, block partials and the finish lanes, in whatever
              fixed order: (n + 2) u sum |dpooled x| (a product one rounding, a sum of n terms n - 1).
Every element is checked against its own bound; nothing is excluded."""
import math

import torch
import torch.nn.functional as F

import ln_ref as lr

U = 2.0 ** -24
BF = 2.0 ** -9
F64 = torch.float64
SLACK2 = 1.0 + 2.0 ** -10           # the second-order remainder of the LayerNorm perturbation
THREADS, MAX_BLOCKS, DW_MAX_BLOCKS, DW_ROWS, TAPS, WLDS_FLOATS = 256, 2048, 256, 4, 9, 8192
CONV, MAX, AVG = 0, 1, 2
MODES = {"conv": CONV, "max": MAX, "avg": AVG}


def bf_round(v):
    """Half a bf16 unit in the last place of any value of magnitude <= v: 2^-9 * 2^ceil(log2 v) (normal range)."""
    return BF * torch.exp2(torch.ceil(torch.log2(v.clamp_min(2.0 ** -126))))


def stored(bound, ref, bf16_out):
    return bound + bf_round(ref.abs() + bound) if bf16_out else bound


# ---- geometry --------------------------------------------------------------------------------------------------------
class Geo:
    def __init__(self, B, thw, k, s, heads, hd, cls, p=None):
        self.B, self.thw, self.k, self.s = B, tuple(thw), tuple(k), tuple(s)
        self.p = tuple(a // 2 for a in k) if p is None else tuple(p)
        self.heads, self.hd, self.cls, self.C = heads, hd, cls, heads * hd
        self.out = tuple((i + 2 * pp - kk) // ss + 1 for i, pp, kk, ss in zip(self.thw, self.p, self.k, self.s))
        self.K = self.k[0] * self.k[1] * self.k[2]
        self.L, self.OL = math.prod(self.thw), math.prod(self.out)
        self.rows_in, self.rows_out = cls + self.L, cls + self.OL

    def taps(self):
        return [(a, b, c) for a in range(self.k[0]) for b in range(self.k[1]) for c in range(self.k[2])]

    def window(self, device="cpu"):
        """cells [K, OL] (the input cell of tap k of output position o, clamped into the grid) and inb [K, OL]."""
        T, H, W = self.thw
        OT, OH, OW = self.out
        ar = lambda n: torch.arange(n, device=device)
        ot, oh, ow = torch.meshgrid(ar(OT), ar(OH), ar(OW), indexing="ij")
        cells, inb = [], []
        for a, b, c in self.taps():
            t, h, w = ot * self.s[0] - self.p[0] + a, oh * self.s[1] - self.p[1] + b, ow * self.s[2] - self.p[2] + c
            ok = (t >= 0) & (t < T) & (h >= 0) & (h < H) & (w >= 0) & (w < W)
            cells.append(((t.clamp(0, T - 1) * H + h.clamp(0, H - 1)) * W + w.clamp(0, W - 1)).reshape(-1))
            inb.append(ok.reshape(-1))
        return torch.stack(cells), torch.stack(inb)

    def cover(self, device="cpu"):
        """The gather form: pos [K, L] (the output position whose tap k is input cell i, clamped) and hit [K, L]:
        (i + p - tap) / s integral and in range, per axis."""
        T, H, W = self.thw
        OT, OH, OW = self.out
        ar = lambda n: torch.arange(n, device=device)
        t, h, w = torch.meshgrid(ar(T), ar(H), ar(W), indexing="ij")
        pos, hit = [], []
        for a, b, c in self.taps():
            ok, o = torch.ones_like(t, dtype=torch.bool), []
            for i, tap, pp, ss, O in ((t, a, self.p[0], self.s[0], OT), (h, b, self.p[1], self.s[1], OH), (w, c, self.p[2], self.s[2], OW)):
                n = i + pp - tap
                q = torch.div(n, ss, rounding_mode="floor")
                ok = ok & (n >= 0) & (n % ss == 0) & (q < O)
                o.append(q.clamp(0, O - 1))
            pos.append(((o[0] * OH + o[1]) * OW + o[2]).reshape(-1))
            hit.append(ok.reshape(-1))
        return torch.stack(pos), torch.stack(hit)

    def wcol(self, device="cpu", div=False):
        """The weight row of every column: col % head_dim (mutant: col / head_dim)."""
        col = torch.arange(self.C, device=device)
        return (col // self.hd) % self.hd if div else col % self.hd


# ---- the references (dtype: fp64; fp32 gives a twin of the kernels' arithmetic) ----------------------------------------
def pool_fwd(x, g, mode, w=None, dtype=F64, tap_perm=None, wdiv=False, avg_inbounds=False, last=False, admit_pad=False):
    """x [B, rows_in, C] -> pooled [B, rows_out, C], idx int8 [B, rows_out, C] (max; -1 on the cls row) or None, and
    scale = sum |w x| per element (the bound's scale; 0 on the cls row and in max mode).
    Mutants: tap_perm (the weight of tap k taken from tap_perm[k]), wdiv (col / head_dim), avg_inbounds (the divisor counts
    the in-bounds taps only), last (the last maximum), admit_pad (a padded tap takes part with the value 0)."""
    dev = x.device
    cells, inb = g.window(dev)
    xs = x.to(dtype)
    body = xs[:, g.cls:]
    B = x.shape[0]
    y = torch.zeros(B, g.OL, g.C, dtype=dtype, device=dev)
    scale = torch.zeros(B, g.OL, g.C, dtype=dtype, device=dev)
    idx = None
    if mode == CONV:
        wc = w.reshape(g.hd, g.K).to(dtype)[g.wcol(dev, wdiv)]                       # [C, K]
    if mode == MAX:
        y.fill_(float("-inf"))
        idx = torch.full((B, g.OL, g.C), -1, dtype=torch.int8, device=dev)
    cnt = inb.sum(0).to(dtype)[None, :, None]
    for k in range(g.K):
        v = body[:, cells[k]]                                                        # [B, OL, C]
        ok = inb[k][None, :, None]
        if mode == MAX:
            if admit_pad:
                v, ok = torch.where(ok, v, torch.zeros_like(v)), torch.ones_like(ok)
            take = ok & (((v >= y) if last else (v > y)) | torch.isnan(v) | (idx < 0))
            y = torch.where(take, v, y)
            idx = torch.where(take, torch.full_like(idx, k), idx)
        else:
            wk = wc[:, k if tap_perm is None else tap_perm[k]] if mode == CONV else torch.full((g.C,), 1.0 / g.K, dtype=dtype, device=dev)
            t = torch.where(ok, v, torch.zeros_like(v))
            if mode == CONV:
                y = y + wk * t
            else:
                y = y + t
            scale = scale + (wk * t).abs()
    if mode == AVG:
        y = y / (cnt if avg_inbounds else torch.tensor(float(g.K), dtype=dtype, device=dev))
    if g.cls:
        y = torch.cat([xs[:, :1], y], 1)
        scale = torch.cat([torch.zeros_like(scale[:, :1]), scale], 1)
        if idx is not None:
            idx = torch.cat([torch.full_like(idx[:, :1], -1), idx], 1)
    return y, idx, scale


def pool_fwd_bound(g, scale, ref, bf16_out, mode):
    """-> (the bound of the un-rounded fp32 value, the bound of the stored value)."""
    e = torch.zeros_like(scale) if mode == MAX else (g.K + 1) * U * scale
    return e, stored(e, ref, bf16_out)


def norm_fwd(pooled, g, gamma, beta, eps):
    """The per-head LayerNorm of pooled [B, rows_out, C] (every row, the cls row included) through ln_ref ->
    y [B, rows_out, C], mean, rstd [B*rows_out*heads] in fp64."""
    y, mean, rstd = lr.fwd(pooled.reshape(-1, g.hd), gamma, beta, eps)
    return y.reshape(pooled.shape), mean, rstd


def norm_fwd_bounds(pooled, e, g, gamma, beta, eps, bf16_out):
    """Bounds of y, mean, rstd: ln_ref's for exact inputs plus the perturbation e of the inputs (the file's docstring)."""
    p2, e2 = pooled.to(F64).reshape(-1, g.hd), e.reshape(-1, g.hd)
    bm, br, by = lr.fwd_bounds(p2, gamma, beta, eps, False)
    y, mean, rstd = lr.fwd(p2, gamma, beta, eps)
    xh = (p2 - mean[:, None]) * rstd[:, None]
    me, mxe = e2.mean(-1), (xh.abs() * e2).mean(-1)
    bm = bm + me
    br = br + SLACK2 * rstd * rstd * mxe
    by = by + SLACK2 * gamma.to(F64).abs() * rstd[:, None] * (e2 + me[:, None] + xh.abs() * mxe[:, None])
    return stored(by, y, bf16_out).reshape(pooled.shape), bm, br


def pool_dx(dp, g, mode, w=None, idx=None, dtype=F64):
    """The gather form: dx [B, rows_in, C] and the sum of |terms| per element."""
    dev = dp.device
    pos, hit = g.cover(dev)
    d = dp.to(dtype)
    body = d[:, g.cls:]
    B = dp.shape[0]
    dx = torch.zeros(B, g.L, g.C, dtype=dtype, device=dev)
    scale = torch.zeros(B, g.L, g.C, dtype=dtype, device=dev)
    if mode == CONV:
        wc = w.reshape(g.hd, g.K).to(dtype)[g.wcol(dev)]
    for k in range(g.K):
        gv = torch.where(hit[k][None, :, None], body[:, pos[k]], torch.zeros((), dtype=dtype, device=dev))
        if mode == CONV:
            t = wc[:, k] * gv
        elif mode == AVG:
            t = gv
        else:
            t = torch.where(idx[:, g.cls:][:, pos[k]] == k, gv, torch.zeros_like(gv))
        dx = dx + t
        scale = scale + t.abs()
    if mode == AVG:
        dx, scale = dx / torch.tensor(float(g.K), dtype=dtype, device=dev), scale / g.K
    if g.cls:
        dx = torch.cat([d[:, :1], dx], 1)
        scale = torch.cat([torch.zeros_like(scale[:, :1]), scale], 1)
    return dx, scale


def pool_dx_bound(g, scale, ref, bf16_out, mode):
    e = (g.K + 1) * U * scale
    return stored(e, ref, bf16_out)


def pool_dw(dp, x, g, dtype=F64):
    """dw [head_dim, K] = the sum over samples, heads and output positions of dpooled * x[tap], and the sum of |terms|."""
    dev = dp.device
    cells, inb = g.window(dev)
    d, xb = dp.to(dtype)[:, g.cls:], x.to(dtype)[:, g.cls:]
    dw, sc = [], []
    for k in range(g.K):
        t = d * torch.where(inb[k][None, :, None], xb[:, cells[k]], torch.zeros((), dtype=dtype, device=dev))
        dw.append(t.sum((0, 1)).view(g.heads, g.hd).sum(0))
        sc.append(t.abs().sum((0, 1)).view(g.heads, g.hd).sum(0))
    return torch.stack(dw, 1), torch.stack(sc, 1)


def pool_dw_bound(g, scale):
    return (g.B * g.heads * g.OL + 2) * U * scale


def window_ties(x, g):
    """Number of (window, column) pairs of x [B, rows_in, C] in which the maximum is attained more than once."""
    y, _, _ = pool_fwd(x, g, MAX)
    cells, inb = g.window(x.device)
    body = x.to(F64)[:, g.cls:]
    cnt = torch.zeros_like(y[:, g.cls:])
    for k in range(g.K):
        cnt += ((body[:, cells[k]] == y[:, g.cls:]) & inb[k][None, :, None]).to(F64)
    return int((cnt > 1).sum())


# ---- the ATen composition: today's attention_pool, permutes and all, in the dtype it is given ---------------------------
def aten_pool(x, g, mode, w=None, norm=None):
    """x [B, rows_in, C] -> [B, rows_out, C] through [B*heads, head_dim, T, H, W], differentiable."""
    B = x.shape[0]
    t = x.reshape(B, g.rows_in, g.heads, g.hd).permute(0, 2, 1, 3)
    if g.cls:
        cls_tok, t = t[:, :, :1], t[:, :, 1:]
    t = t.reshape(B * g.heads, *g.thw, g.hd).permute(0, 4, 1, 2, 3).contiguous()
    if mode == CONV:
        t = F.conv3d(t, w.reshape(g.hd, 1, *g.k), None, g.s, g.p, 1, g.hd)
    elif mode == MAX:
        t = F.max_pool3d(t, g.k, g.s, g.p)
    else:
        t = F.avg_pool3d(t, g.k, g.s, g.p)
    t = t.reshape(B, g.heads, g.hd, g.OL).transpose(2, 3)
    if g.cls:
        t = torch.cat((cls_tok, t), 2)
    if norm is not None:
        t = F.layer_norm(t, (g.hd,), norm[0], norm[1], norm[2])
    return t.permute(0, 2, 1, 3).reshape(B, g.rows_out, g.C)


# ---- the walk of the grids: a transcription of the host side of csrc/token_pool.hip ----------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def pow2_up(v):
    p = 1
    while p < v:
        p *= 2
    return p


def fwd_lanes(g, norm):
    ug = g.hd // 8 if norm else 1
    return g.B * g.rows_out * (g.C // (8 * ug)) * pow2_up(ug)


def fwd_blocks(g, norm):
    return min(max(_cdiv(fwd_lanes(g, norm), THREADS), 1), MAX_BLOCKS)


def dx_blocks(g):
    return min(max(_cdiv(g.B * g.rows_in * (g.C // 8), THREADS), 1), MAX_BLOCKS)


def dw_tiles(g):
    return _cdiv(g.C // 8, min(g.C // 8, THREADS))


def dw_blocks(g):
    rl = THREADS // min(g.C // 8, THREADS)
    return min(max(_cdiv(g.B * g.OL, rl * DW_ROWS), 1), DW_MAX_BLOCKS)


def workspace_bytes(g):
    return (dw_blocks(g) * dw_tiles(g) * g.hd * g.K * 4 + 15) // 16 * 16


def blocks(g, stage):
    """focus_token_pool_blocks."""
    return fwd_blocks(g, stage == 1) if stage <= 1 else dx_blocks(g) if stage == 2 else dw_blocks(g)


# ---- the case table -----------------------------------------------------------------------------------------------------
# thw, kernel, stride, mode, heads, head_dim, cls, norm; padding is kernel // 2 (attention.py:188-189, :266); xrs: the row
# stride of x in units of C (a column block of a wider matrix)
def _case(thw, k, s, mode, heads, hd, cls, norm, xrs=1, B=2):
    return dict(thw=thw, k=k, s=s, mode=mode, heads=heads, hd=hd, cls=cls, norm=norm, xrs=xrs, B=B)


CASES = [
    _case((2, 5, 7), (3, 3, 3), (1, 2, 2), "conv", 2, 16, 1, True),
    _case((3, 4, 4), (3, 3, 3), (1, 8, 8), "conv", 1, 96, 1, True),
    _case((2, 3, 3), (3, 3, 3), (1, 1, 1), "conv", 3, 8, 0, True),
    _case((4, 6, 5), (3, 3, 3), (2, 2, 2), "conv", 1, 24, 1, False),
    _case((2, 4, 6), (1, 1, 1), (1, 2, 2), "conv", 2, 8, 1, True),
    _case((2, 5, 7), (1, 3, 3), (1, 2, 2), "max", 1, 32, 1, False),
    _case((3, 5, 4), (3, 3, 3), (1, 2, 2), "max", 2, 8, 1, False),
    _case((3, 5, 4), (3, 3, 3), (1, 2, 2), "avg", 2, 8, 1, False),
    _case((1, 1, 1), (3, 3, 3), (1, 2, 2), "conv", 1, 8, 1, True),
]
N_ISSUE = len(CASES)
CASES += [
    _case((2, 5, 7), (3, 3, 3), (1, 2, 2), "conv", 2, 16, 1, True, xrs=3),       # a strided input view
    _case((2, 5, 5), (3, 5, 5), (1, 2, 2), "conv", 1, 128, 1, True),             # head_dim * taps > 8192: weights not in LDS
    _case((2, 3, 3), (1, 3, 3), (1, 2, 2), "conv", 20, 104, 1, True),            # 260 channel groups: two dw tiles
    _case((2, 4, 4), (1, 3, 3), (1, 2, 2), "max", 1, 768, 1, False),             # the skip pool: head_dim = C above 128
    _case((3, 5, 4), (3, 3, 3), (1, 2, 2), "avg", 2, 8, 0, True),                # avg with the norm, no cls
]


def case_id(c):
    return "%dx%dx%d-k%d%d%d-s%d%d%d-%s-%dx%d-cls%d-%s%s" % (*c["thw"], *c["k"], *c["s"], c["mode"], c["heads"], c["hd"], c["cls"],
                                                             "norm" if c["norm"] else "plain", "-xrs%d" % c["xrs"] if c["xrs"] > 1 else "")


def geo_of(c):
    return Geo(c["B"], c["thw"], c["k"], c["s"], c["heads"], c["hd"], c["cls"])


def big_case(blocks_fn):
    """The smallest H (W = H + 1, T = 4) of a 1x3x3 stride-1 conv at 1 x 128 with the norm whose forward walks its grid-stride
    loop twice and whose dw partials exceed one wave; blocks_fn(geo, stage): focus_token_pool_blocks."""
    H = 8
    while True:
        c = _case((4, H, H + 1), (1, 3, 3), (1, 1, 1), "conv", 1, 128, 1, True)
        g = geo_of(c)
        if fwd_lanes(g, True) > blocks_fn(g, 1) * THREADS and blocks_fn(g, 3) > 64:
            return c
        H += 8


EPS = 1e-6


def no_tie_map(g, gen, device="cpu"):
    """[B, rows_in, C] of per-(sample, column) random permutations of the integers -L/2 .. L/2 - 1 (the cls row 0.5): distinct
    in every window and exact in bf16 (L <= 256)."""
    assert g.L <= 256
    perm = torch.rand(g.B, g.L, g.C, generator=gen).argsort(dim=1).float() - g.L // 2
    x = torch.cat([torch.full((g.B, g.cls, g.C), 0.5), perm], 1)
    assert torch.equal(x.bfloat16().float(), x)
    return x.to(device)


def inputs(c, dtype, seed, device="cpu"):
    """x (rounded to `dtype`; max mode: the no-tie map), w [hd, 1, kt, kh, kw], gamma (column 1 zero), beta (fp32), the
    cotangent dy [B, rows_out, C] (rounded to `dtype`)."""
    g = geo_of(c)
    gen = torch.Generator().manual_seed(seed * 7919 + g.L * 31 + g.C)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = no_tie_map(g, gen) if c["mode"] == "max" else rn(g.B, g.rows_in, g.C) * 1.5 + 0.25
    gamma = rn(g.hd)
    gamma[1] = 0.0
    t = dict(x=x.to(dtype), w=rn(g.hd, 1, *g.k) * 0.5, gamma=gamma, beta=rn(g.hd), dy=rn(g.B, g.rows_out, g.C).to(dtype))
    return {k: v.to(device) for k, v in t.items()}


def worst_ratio(got, want, bound):
    return lr.worst_ratio(got, want, bound)
