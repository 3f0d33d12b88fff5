"""The RoI head pooling in fp64, the bounds its fp32 kernels have to keep, an fp32 restatement of the kernels' order, mutants,
and the case table.

    pooled[k, c] = max over bins of RoIAlign(mean_t x[b_k, t, :, :, c])          (head_helper.py:103-118)

No GPU code and no import of focus_amd: tests/test_roi_head_ref_cpu.py checks this file on the CPU (against the oracle's
RoIAlign, against torch.autograd, the restatement inside the bounds, every mutant outside them); tests/test_gpu_roi_head.py
runs csrc/roi_head.hip against it.

What is fp32 by contract.  The sample coordinates (box * scale - 0.5, bin sizes, the adaptive grid ceil(roi / bins), the
sample points) are computed operation by operation in fp32 as oracle/roi_align_ref.c does: grid sizes and neighbour indices are
integers that have to agree bit for bit (focus_roi_align_indices), so the twin takes the same fp32 coordinates.  Everything
downstream of them -- the bilinear weights, the temporal mean, the sums, the division by count -- is fp64 here.

Bounds (u = 2^-24; first order in u).  Inputs are exact: the tests round x and dpooled to the storage type first.
forward, per (box k, channel c), X = max |x[b_k, :, :, :, c]|:
  mean    m = (sum over T terms in order) / T: (T - 1) u for the sum, u for the division: |d m| <= T u X.
  weights the fractional part ly = y - y_low of an fp32 coordinate is exact; hy = 1 - ly: u; a product hy hx: u more.
          rel(w) <= 3 u.  The four weights of a sample are >= 0 and sum to 1 (exactly, before rounding).
  bin     v = (sum over grid_h grid_w samples of ((w1 a + w2 b) + w3 c) + w4 d) / count: every product u, at most
          4 grid_h grid_w additions, the division u.  With sum of weights / count <= 1:
              |d v| <= (T + 3 + 1 + 4 grid_h grid_w + 1) u X  =  (T + 4 grid_h grid_w + 5) u X.
          (The value is a combination of at most T 4 grid_h grid_w inputs with non-negative weights summing to <= 1; the
          count above is the number of roundings on the longest path through it, which is what multiplies u X.)
  pooled  the max of computed values differs from the max of exact values by at most the largest bin error: the same bound.
          A bf16 pooled is rounded to nearest once more (8 significant bits): + 2^-8 (|pooled| + the bound so far).
  arg     is checked by value: the exact value of the bin a kernel chose is within 2 x the bin bound of the exact maximum
          (its computed value was >= the computed value of the exact winner; each is off by at most the bound).
backward, per (image b, cell, channel c), from a given arg.  A term is (dp / count) w: the division u, w 3 u, the product u;
  the terms of a cell are added in a fixed order, n_b = sum over the boxes of image b of 4 grid_h grid_w additions at most;
  the division by T: u.  With S = the same sum over |dp| (weights are >= 0, so S is the sum of the absolute terms) / T:
              |d dx| <= (n_b + 6) u S.        bf16: + 2^-8 (|dx| + that).
Every element is checked against its own bound; nothing is excluded."""
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
BF = 2.0 ** -8
F32 = np.float32


# ---- geometry: fp32, operation by operation (oracle/roi_align_ref.c geometry / sample_y / locate) --------------------------
def geometry(roi4, scale, PH, PW, sampling_ratio, aligned, shift=True, fixed_count=None):
    """roi4: x1, y1, x2, y2.  `shift` False drops the -0.5 of `aligned` (mutant); fixed_count replaces count (mutant)."""
    r = np.asarray(roi4, dtype=F32)
    s = F32(scale)
    off = F32(0.5) if (aligned and shift) else F32(0.0)
    x1, y1, x2, y2 = (r[i] * s - off for i in range(4))
    rw, rh = F32(x2 - x1), F32(y2 - y1)
    if not aligned:
        rw, rh = max(rw, F32(1.0)), max(rh, F32(1.0))
    bin_h, bin_w = F32(rh / F32(PH)), F32(rw / F32(PW))
    gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(F32(rh / F32(PH)))))
    gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(F32(rw / F32(PW)))))
    count = max(gh * gw, 1) if fixed_count is None else fixed_count
    return dict(x1=F32(x1), y1=F32(y1), bin_h=bin_h, bin_w=bin_w, gh=gh, gw=gw, count=count)


def _coords(start, P, bin_, grid):
    """[P, grid] fp32 sample coordinates start + p*bin + (i + 0.5)*bin/grid, left to right."""
    p = np.arange(P, dtype=F32)[:, None]
    i = np.arange(max(grid, 0), dtype=F32)[None, :]
    return ((start + p * bin_).astype(F32) + (((i + F32(0.5)) * bin_).astype(F32) / F32(max(grid, 1))).astype(F32)).astype(F32)


def _locate1(v, L):
    """One axis of locate(): fp32 coordinates [...] -> valid, low, high (int), l (the fp32 fractional part, exact)."""
    valid = ~((v < F32(-1.0)) | (v > F32(L)))
    v = np.where(v <= 0, F32(0.0), v).astype(F32)
    low = v.astype(np.int64)
    top = low >= L - 1
    low = np.where(top, L - 1, low)
    high = np.where(top, L - 1, low + 1)
    v = np.where(top, low.astype(F32), v).astype(F32)
    l = (v - low.astype(F32)).astype(F32)
    low, high = np.where(valid, low, 0), np.where(valid, high, 0)
    return valid, low, high, l


def axis_matrix(start, P, bin_, grid, L):
    """A [P, L] fp64: the summed 1-D bilinear weights of bin row p on cell y (invalid samples contribute nothing)."""
    A = np.zeros((P, L), np.float64)
    if grid <= 0:
        return A
    valid, low, high, l = _locate1(_coords(start, P, bin_, grid), L)
    l = l.astype(np.float64)
    for p in range(P):
        for i in range(grid):
            if valid[p, i]:
                A[p, low[p, i]] += 1.0 - l[p, i]
                A[p, high[p, i]] += l[p, i]
    return A


def bin_matrix(roi4, scale, PH, PW, sampling_ratio, aligned, H, W, **mut):
    """Wbin [PH*PW, H*W] fp64 (already divided by count), and the geometry.  A sample is valid iff both its coordinates are, and
    its weight on cell (y, x) is wy(y) wx(x), so the matrix is the outer product of the two axis matrices."""
    g = geometry(roi4, scale, PH, PW, sampling_ratio, aligned, **mut)
    Ay = axis_matrix(g["y1"], PH, g["bin_h"], g["gh"], H)
    Ax = axis_matrix(g["x1"], PW, g["bin_w"], g["gw"], W)
    Wb = np.einsum("py,qx->pqyx", Ay, Ax).reshape(PH * PW, H * W) / g["count"]
    return Wb, g


def indices(rois5, scale, PH, PW, sampling_ratio, aligned, H, W):
    """grid [K,2], nbr [K,PH,PW,4] of sample (0, 0): what focus_roi_align_indices exports."""
    K = len(rois5)
    grid, nbr = np.zeros((K, 2), np.int32), np.full((K, PH, PW, 4), -1, np.int32)
    for k in range(K):
        g = geometry(rois5[k][1:], scale, PH, PW, sampling_ratio, aligned)
        grid[k] = (g["gh"], g["gw"])
        if g["gh"] <= 0 or g["gw"] <= 0:
            continue
        vy, ly, hy, _ = _locate1(_coords(g["y1"], PH, g["bin_h"], g["gh"])[:, 0], H)
        vx, lx, hx, _ = _locate1(_coords(g["x1"], PW, g["bin_w"], g["gw"])[:, 0], W)
        ok = vy[:, None] & vx[None, :]
        for j, a in enumerate((np.broadcast_to(ly[:, None], ok.shape), np.broadcast_to(lx[None, :], ok.shape),
                               np.broadcast_to(hy[:, None], ok.shape), np.broadcast_to(hx[None, :], ok.shape))):
            nbr[k, :, :, j] = np.where(ok, a, -1)
    return grid, nbr


# ---- the reference ------------------------------------------------------------------------------------------------------
def fwd(x, rois5, T, H, W, PH, PW, scale, sampling_ratio=0, aligned=True, reduce="max", t_div=None, **mut):
    """x [B, T*H*W, C] (patch tokens, any float type), rois5 [K,5] -> pooled [K,C], bins [K,PH*PW,C], arg [K,C] in fp64 / int64.
    The lowest bin wins a tie.  reduce / t_div / **mut: the mutants."""
    x = np.asarray(x.detach().cpu().to(torch.float64))
    B, _, C = x.shape
    mean = x.reshape(B, T, H * W, C).sum(1) / (T if t_div is None else t_div)
    r = np.asarray(rois5, dtype=np.float64)
    K = r.shape[0]
    bins = np.zeros((K, PH * PW, C), np.float64)
    for k in range(K):
        Wb, _ = bin_matrix(r[k, 1:], scale, PH, PW, sampling_ratio, aligned, H, W, **mut)
        bins[k] = Wb @ mean[int(r[k, 0])]
    arg = bins.argmax(1)
    pooled = bins.max(1) if reduce == "max" else bins.mean(1)
    return pooled, bins, arg


def bwd(dp, arg, rois5, B, T, H, W, PH, PW, scale, sampling_ratio=0, aligned=True, div_t=True, absolute=False):
    """dpooled [K,C], a GIVEN arg [K,C] -> dx [B, T*H*W, C] fp64.  absolute: the same sum over |dp| (the bound's S)."""
    dp = np.asarray(dp.detach().cpu().to(torch.float64)) if isinstance(dp, torch.Tensor) else np.asarray(dp, np.float64)
    if absolute:
        dp = np.abs(dp)
    arg = np.asarray(arg.cpu() if isinstance(arg, torch.Tensor) else arg).astype(np.int64)
    r = np.asarray(rois5, dtype=np.float64)
    K, C = dp.shape
    dmean = np.zeros((B, H * W, C), np.float64)
    for k in range(K):
        Wb, _ = bin_matrix(r[k, 1:], scale, PH, PW, sampling_ratio, aligned, H, W)
        dmean[int(r[k, 0])] += (Wb[arg[k]] * dp[k][:, None]).T          # [cells, C]
    if div_t:
        dmean = dmean / T
    return np.broadcast_to(dmean[:, None], (B, T, H * W, C)).reshape(B, T * H * W, C).copy()


# ---- the bounds ---------------------------------------------------------------------------------------------------------
def fwd_bound(x, rois5, T, H, W, PH, PW, scale, sampling_ratio, aligned, bf16_out, pooled=None):
    """-> [K, C] absolute bound of a bin value / of pooled (bf16_out adds the output rounding, which needs `pooled`)."""
    x = np.asarray(x.detach().cpu().to(torch.float64))
    B, _, C = x.shape
    X = np.abs(x).max(1)                                                  # [B, C]
    r = np.asarray(rois5, dtype=np.float64)
    out = np.zeros((r.shape[0], C), np.float64)
    for k in range(r.shape[0]):
        g = geometry(r[k, 1:], scale, PH, PW, sampling_ratio, aligned)
        out[k] = (T + 4 * max(g["gh"], 0) * max(g["gw"], 0) + 5) * U * X[int(r[k, 0])]
    if bf16_out:
        out = out + BF * (np.abs(pooled) + out)
    return out


def bwd_bound(dp, arg, rois5, B, T, H, W, PH, PW, scale, sampling_ratio, aligned, bf16_out, dx=None):
    r = np.asarray(rois5, dtype=np.float64)
    n = np.zeros(B)
    for k in range(r.shape[0]):
        g = geometry(r[k, 1:], scale, PH, PW, sampling_ratio, aligned)
        n[int(r[k, 0])] += 4 * max(g["gh"], 0) * max(g["gw"], 0)
    S = bwd(dp, arg, rois5, B, T, H, W, PH, PW, scale, sampling_ratio, aligned, absolute=True)
    b = (n[:, None, None] + 6) * U * S
    if bf16_out:
        b = b + BF * (np.abs(dx) + b)
    return b


def worst_ratio(got, want, bound):
    """Largest |got - want| / bound; an element whose bound is 0 has to be exact.  NaN or Inf count as infinite."""
    got = np.asarray(got.detach().cpu().to(torch.float64)) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    e = np.abs(got - want)
    e = np.where(np.isfinite(e), e, math.inf)
    zero = bound == 0
    if (e[zero] != 0).any():
        return math.inf
    if zero.all():
        return 0.0
    return float((e[~zero] / bound[~zero]).max())


def arg_ratio(arg, bins, bound):
    """The exact value of the chosen bin against the exact maximum, over 2 x the bin bound (see `arg` above)."""
    arg = np.asarray(arg.cpu() if isinstance(arg, torch.Tensor) else arg).astype(np.int64)
    if (arg < 0).any() or (arg >= bins.shape[1]).any():
        return math.inf
    chosen = np.take_along_axis(bins, arg[:, None, :], 1)[:, 0]
    return worst_ratio(chosen, bins.max(1), 2 * bound)


# ---- fp32 restatement of the kernels' accumulation order (csrc/roi_head.hip) ---------------------------------------------
def twin_fwd(x, rois5, T, H, W, PH, PW, scale, sampling_ratio=0, aligned=True):
    """x [B, T*H*W, C] in its storage type -> pooled [K,C] (rounded to that type, as float64 values), arg [K,C]: the mean as a
    sum over t in order and one division; per bin, samples in (iy, ix) order, acc += ((w1 a + w2 b) + w3 c) + w4 d with fp32
    weights, no fused multiply-add; the division by count; the lowest bin among equal maxima."""
    dt = x.dtype
    xf = x.detach().cpu().float().numpy()
    B, _, C = xf.shape
    xf = xf.reshape(B, T, H, W, C)
    mean = np.zeros((B, H, W, C), F32)
    for t in range(T):
        mean = (mean + xf[:, t]).astype(F32)
    mean = (mean / F32(T)).astype(F32)
    r = np.asarray(rois5, dtype=np.float64)
    K = r.shape[0]
    pooled, arg = np.zeros((K, C), F32), np.zeros((K, C), np.int64)
    for k in range(K):
        g = geometry(r[k, 1:], scale, PH, PW, sampling_ratio, aligned)
        m = mean[int(r[k, 0])]
        acc = np.zeros((PH, PW, C), F32)
        if g["gh"] > 0 and g["gw"] > 0:
            vy, yl, yh, ly = _locate1(_coords(g["y1"], PH, g["bin_h"], g["gh"]), H)
            vx, xl, xh, lx = _locate1(_coords(g["x1"], PW, g["bin_w"], g["gw"]), W)
            hy, hx = (F32(1.0) - ly).astype(F32), (F32(1.0) - lx).astype(F32)
            for iy in range(g["gh"]):
                for ix in range(g["gw"]):
                    ok = (vy[:, iy][:, None] & vx[:, ix][None, :])[:, :, None]
                    w = [(a[:, iy][:, None] * b[:, ix][None, :]).astype(F32)[:, :, None]
                         for a, b in ((hy, hx), (hy, lx), (ly, hx), (ly, lx))]
                    Y0, Y1, X0, X1 = yl[:, iy][:, None], yh[:, iy][:, None], xl[:, ix][None, :], xh[:, ix][None, :]
                    s = (w[0] * m[Y0, X0]).astype(F32)
                    s = (s + (w[1] * m[Y0, X1]).astype(F32)).astype(F32)
                    s = (s + (w[2] * m[Y1, X0]).astype(F32)).astype(F32)
                    s = (s + (w[3] * m[Y1, X1]).astype(F32)).astype(F32)
                    acc = np.where(ok, (acc + s).astype(F32), acc)
        v = (acc / F32(g["count"])).astype(F32).reshape(PH * PW, C)
        arg[k] = v.argmax(0)
        pooled[k] = v.max(0)
    return torch.from_numpy(pooled).to(dt).to(torch.float64).numpy(), arg


def twin_bwd(dp, arg, rois5, B, T, H, W, PH, PW, scale, sampling_ratio=0, aligned=True):
    """The backward kernel's order in fp32: per (image, channel) the boxes in index order, gv = dp / count, the samples of bin
    arg in (iy, ix) order, the four cells of a sample in turn += gv * w (fp32 weights), then / T.  -> dx [B, T*H*W, C] as float64
    values of the storage type."""
    dt = dp.dtype
    dpf = dp.detach().cpu().float().numpy()
    arg = np.asarray(arg.cpu() if isinstance(arg, torch.Tensor) else arg).astype(np.int64)
    r = np.asarray(rois5, dtype=np.float64)
    K, C = dpf.shape
    slab = np.zeros((B, H * W, C), F32)
    for k in range(K):
        g = geometry(r[k, 1:], scale, PH, PW, sampling_ratio, aligned)
        if g["gh"] <= 0 or g["gw"] <= 0:
            continue
        b = int(r[k, 0])
        vy, yl, yh, ly = _locate1(_coords(g["y1"], PH, g["bin_h"], g["gh"]), H)
        vx, xl, xh, lx = _locate1(_coords(g["x1"], PW, g["bin_w"], g["gw"]), W)
        hy, hx = (F32(1.0) - ly).astype(F32), (F32(1.0) - lx).astype(F32)
        gv = (dpf[k] / F32(g["count"])).astype(F32)
        for a in np.unique(arg[k]):
            ch = np.nonzero(arg[k] == a)[0]
            ph, pw = int(a) // PW, int(a) % PW
            for iy in range(g["gh"]):
                for ix in range(g["gw"]):
                    if not (vy[ph, iy] and vx[pw, ix]):
                        continue
                    for cy, cx, w in ((yl, xl, hy[ph, iy] * hx[pw, ix]), (yl, xh, hy[ph, iy] * lx[pw, ix]),
                                      (yh, xl, ly[ph, iy] * hx[pw, ix]), (yh, xh, ly[ph, iy] * lx[pw, ix])):
                        cell = int(cy[ph, iy]) * W + int(cx[pw, ix])
                        slab[b, cell, ch] = (slab[b, cell, ch] + (gv[ch] * F32(w)).astype(F32)).astype(F32)
    slab = (slab / F32(T)).astype(F32)
    dx = np.broadcast_to(slab[:, None], (B, T, H * W, C)).reshape(B, T * H * W, C)
    return torch.from_numpy(dx.copy()).to(dt).to(torch.float64).numpy()


# ---- the case table -----------------------------------------------------------------------------------------------------
B = 3
SCALE_FACTOR = 16                     # input pixels per feature cell


def boxes(H, W):
    """K = 9 boxes (batch index, x1, y1, x2, y2) in input pixels for an H x W map at 16 pixels per cell, in shuffled batch
    order, image 1 without any: whole frame; smaller than one bin (grid 1); adaptive grid >= 3 (with 3 x 2 bins: the whole
    frame, and this one, a box of 9+ cells per bin at 14 x 14); over the right and bottom edge; entirely outside; zero area;
    three ordinary ones."""
    s, w, h = float(SCALE_FACTOR), W * float(SCALE_FACTOR), H * float(SCALE_FACTOR)
    return np.array([
        [2, 0.0, 0.0, w, h],                                    # the whole frame
        [0, 1.3 * s, 2.1 * s, 1.3 * s + 5.0, 2.1 * s + 4.0],    # smaller than one bin of any table entry
        [2, 0.5 * s, 0.25 * s, w - 3.0, h - 7.0],               # nearly the frame, off the cell lattice
        [0, w - 2.2 * s, h - 1.7 * s, w + 1.5 * s, h + 2.5 * s],  # hangs over the right and bottom edge
        [2, w + 3.0 * s, h + 3.0 * s, w + 5.0 * s, h + 6.0 * s],  # entirely outside: zeros, arg 0
        [0, 2.0 * s, 3.0 * s, 2.0 * s, 3.0 * s],                # zero area
        [0, 0.7 * s, 1.1 * s, 0.7 * s + 0.55 * w, 1.1 * s + 0.5 * h],
        [2, 0.2 * w, 0.3 * h, 0.9 * w, 0.8 * h],
        [0, -1.5 * s, -0.6 * s, 0.4 * w, 0.6 * h],              # starts left of and above the frame
    ], dtype=np.float32)


def _build():
    Ts, maps, Cs, Ps = (1, 2, 8), ((7, 7), (5, 9), (14, 14)), (8, 40, 96), ((7, 7), (3, 2))
    cs, i = [], 0
    for dtype in ("fp32", "bf16"):
        for ti, T in enumerate(Ts):
            for mi, (H, W) in enumerate(maps):
                for pi, (PH, PW) in enumerate(Ps):
                    n = i // 2                                            # the (dtype, T, map) combination
                    cs.append(dict(dtype=dtype, T=T, H=H, W=W, C=Cs[(ti + mi + pi) % 3], PH=PH, PW=PW, cls=(n + pi) % 2,
                                   aligned=(n // 2 + pi) % 2, sr=(0, 2)[(ti + mi + pi + (dtype == "bf16")) % 2]))
                    i += 1
    return cs


CASES = _build()


def case_id(c):
    return "%s-T%d-%dx%d-C%d-P%dx%d-cls%d-al%d-sr%d" % (c["dtype"], c["T"], c["H"], c["W"], c["C"], c["PH"], c["PW"], c["cls"],
                                                        c["aligned"], c["sr"])


def torch_dtype(c):
    return torch.float32 if c["dtype"] == "fp32" else torch.bfloat16


def inputs(c):
    """-> x [B, T*H*W, C] and dp [K, C] rounded to the storage type, rois [K,5] fp32 (numpy)."""
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    dt = torch_dtype(c)
    x = (torch.randn(B, c["T"] * c["H"] * c["W"], c["C"], generator=g) * 1.5 + 0.25).to(dt)
    rois = boxes(c["H"], c["W"])
    dp = torch.randn(rois.shape[0], c["C"], generator=g).to(dt)
    return x, dp, rois


def args_of(c):
    return dict(T=c["T"], H=c["H"], W=c["W"], PH=c["PH"], PW=c["PW"], scale=1.0 / SCALE_FACTOR, sampling_ratio=c["sr"],
                aligned=bool(c["aligned"]))


# ---- inputs whose top two bins are separated ----------------------------------------------------------------------------
def separated_inputs(T=2, H=7, W=7, C=8, PH=3, PW=2, seed=0, dtype=torch.float32):
    """Per channel a plane a_c (y - yc) + b_c (x - xc) through the map centre (|a_c|, |b_c| in [0.8, 1.2], every sign pattern)
    times a per-frame factor of mean 1 and a per-image factor (1, -0.8), plus noise of 1e-3: RoIAlign of a plane is the plane at
    the bin centres, so the maximum sits in a corner bin and leads the runner-up by min(|a_c| bin_h, |b_c| bin_w) times the image
    factor.  Boxes inside the frame with bins of >= 0.7 cell: the lead is >= 0.8 * 0.7 * 0.8 = 0.448 less the noise, while
    |x| <= 1.2 * 6 * 1.1 < 8.  -> x [B, T*H*W, C], rois [K,5] (numpy fp32), B."""
    g = torch.Generator().manual_seed(seed)
    Bn = 2
    sign = torch.tensor([[1, 1], [1, -1], [-1, 1], [-1, -1]], dtype=torch.float64)[torch.arange(C) % 4]
    ab = (0.8 + 0.4 * torch.rand(C, 2, generator=g, dtype=torch.float64)) * sign
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    plane = (yy - (H - 1) / 2.0)[:, :, None] * ab[:, 0] + (xx - (W - 1) / 2.0)[:, :, None] * ab[:, 1]                           # [H, W, C]
    ft = 1.0 + 0.2 * (torch.arange(T, dtype=torch.float64) - (T - 1) / 2.0)
    x = plane[None, None] * ft[None, :, None, None, None] * torch.tensor([1.0, -0.8], dtype=torch.float64)[:, None, None, None, None]
    x = x + 1e-3 * torch.randn(Bn, T, H, W, C, generator=g, dtype=torch.float64)
    s = float(SCALE_FACTOR)
    rois = np.array([[1, 1.0 * s, 1.2 * s, 1.0 * s + PW * 0.9 * s, 1.2 * s + PH * 1.1 * s],
                     [0, 0.8 * s, 0.6 * s, 0.8 * s + PW * 2.3 * s, 0.6 * s + PH * 1.7 * s],
                     [1, 2.1 * s, 0.9 * s, 2.1 * s + PW * 0.7 * s, 0.9 * s + PH * 0.8 * s]], dtype=np.float32)
    return x.reshape(Bn, T * H * W, C).to(dtype), rois, Bn


def separation(bins):
    """Smallest lead of the largest bin over the second largest, over all (k, c)."""
    s = np.sort(bins, axis=1)
    return float((s[:, -1] - s[:, -2]).min())
