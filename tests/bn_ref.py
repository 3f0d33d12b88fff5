"""BatchNorm2d / MaxPool2d(3, 2, 1) over channels-last rows in fp64, the bounds the fp32 kernels of csrc/batchnorm.hip have to
keep, the walk of their reductions, a plain torch.nn restatement of STEVE's ResNet-18 trunk, the case table and mutants.

No GPU code and no import of focus_amd: tests/test_bn_ref_cpu.py checks this file on the CPU (the references against
torch.nn.functional and autograd, an fp32 twin of every stage against the bounds, every mutant outside them);
tests/test_gpu_batchnorm.py runs the kernels against it.

Bounds (u = 2^-24, first order in u unless said otherwise).  A bf16 output is rounded to nearest once more: half a unit in
the last place, 2^-9 of the power of two that closes the value's binade from above (bf_round(); relative to the value itself
that is up to 2^-8, which is what tests/ln_ref.py charges: the bound here is the tighter of the two and exact).
Inputs are exact: the tests round x, dy, residual to the storage type first; parameters and statistics are fp32.

statistics, per channel.  The kernel is a tree of merges of (count, mean, M2) triples: a thread's Welford steps over its k
  rows (a merge with a single element), the RPB - 1 sequential merges of a workgroup's row lanes, a lane's ceil(nblk / 64)
  sequential merges of block partials and 6 tree steps.  L = k + RPB - 1 + ceil(nblk / 64) + 6 bounds the merges on any path
  (stats_walk() below walks the same tree in fp64).  With A = max |x|, S = max x - min x of the channel:
  mean   a merge forms m = ma + (mb - ma) f, f = nb / n: the difference is off by u S, f by 2u, the product by u S, the sum by
         u A; the errors of ma and mb enter as a convex combination.  |d_mean| <= L u (A + 4 S) =: dm.
  M2     the exact identity is M2 = sum over all merges of d^2 w (d = mb - ma, w = na nb / n): every term is >= 0.
         rounding: a term is off by 6u relative and passes through at most 2L additions: (2L + 6) u M2.
         the means: a merge that is handed means off by da, db computes a sum of squares that is off by 2 d w (da - db) at
         FIRST order (the part a shifted mean moves is not zero inside a subset), so by at most 4 dm T1 over the tree with
         T1 = sum over all merges of |d| w, which stats_walk() returns for the data at hand; second order R dm^2.
         |d_M2| <= (2L + 6) u M2 + 4 dm T1 + R dm^2.
         (E[x^2] - E[x]^2 is off by about R u A^2 instead: the `naive` mutant.)
  rstd   v = M2 / R + eps: rel(v) = (d_M2 / R) / (var + eps) + 2u; 1 / sqrt(v), stored: rel(rstd) = rel(v) (1 + rel(v)) / 2 + 5u.
  running r' = (1 - mom) r + mom s: |mom| ds + 4u (|(1 - mom) r| + |mom s|), ds = dm for the mean and
         d_M2 / (R - 1) + 2u M2 / (R - 1) for the unbiased variance.
apply, per element, from the fp32 mean and rstd it is given: t = x - mean (u |t|), s = gamma rstd (u), t s + beta (2u |t s| and
  u of the sum, fused or not), + residual (u of the sum); ReLU is exact and does not expand an error:
  3u |t s| + u |t s + beta| + u |y| (residual) [+ bf_round(|y| + that)].
backward, from the fp32 mean, rstd and the STORED y (so g = dy or 0 is exact):
  x^ = (x - mean) rstd is off by 2u relative, a term g x^ by 3u.  A sum over the rows passes through at most
  Ls = k + RPB + ceil(nblk / 16) + 16 additions: |d_dbeta| <= Ls u sum |g|, |d_dgamma| <= (Ls + 3) u sum |g x^|.
  k1 = dbeta / R and k2 = dgamma / R (a product with the rounded 1 / R: 2u): e1 = d_dbeta / R + 2u |k1|, e2 likewise.
  dx = a (g - k1 - x^ k2), a = gamma rstd:  |a| [e1 + |x^| e2 + 3u |x^ k2| + 2u (|g| + |k1| + |x^ k2|)] + 2u |dx|
  [+ bf_round(|dx| + that)];  frozen: dx = a g, 2u |dx| [+ bf_round].  dres = g bit for bit.
max-pool: y and idx are exact; the backward sums at most 4 terms: 3u sum |terms| [+ bf_round(|dx| + that)].
Every element is checked against its own bound; nothing is excluded."""
import torch
import torch.nn as nn
import torch.nn.functional as F

U = 2.0 ** -24
BF = 2.0 ** -9
F64 = torch.float64
THREADS, UNROLL, MAX_BLOCKS = 256, 4, 1024


def bf_round(v):
    """Half a bf16 unit in the last place of any value of magnitude <= v: 2^-9 * 2^ceil(log2 v) (normal range)."""
    return BF * torch.exp2(torch.ceil(torch.log2(v.clamp_min(2.0 ** -126))))


# ---- the walk of the kernels' reductions: a transcription of csrc/batchnorm.hip ------------------------------------------
def blocks(R):
    """focus_bn_blocks."""
    return max(1, min(MAX_BLOCKS, -(-R // 32)))


def rpb(C):
    """Row lanes of a workgroup: 256 threads / (C / 8) channel groups."""
    return THREADS // (C // 8)


def rows_per_thread(R, C):
    return -(-R // (blocks(R) * rpb(C)))


def workspace_bytes(R, C):
    return (blocks(R) * (2 * C + 1) * 4 + 15) // 16 * 16


def depth_stats(R, C):
    return rows_per_thread(R, C) + rpb(C) - 1 + -(-blocks(R) // 64) + 6


def depth_sums(R, C):
    return rows_per_thread(R, C) + rpb(C) + -(-blocks(R) // 16) + 16


def _merge(a, b):
    """Chan's merge of (n, mean, M2, T1) with (n, mean, M2, T1); an empty b changes nothing."""
    na, ma, qa, ta = a
    nb, mb, qb, tb = b
    n = na + nb
    f = torch.where(n > 0, nb / n.clamp_min(1), torch.zeros_like(n))
    d = torch.where(nb > 0, mb - ma, torch.zeros_like(ma))
    w = na * f
    return n, ma + d * f, qa + qb + d * d * w, ta + tb + d.abs() * w


def stats_walk(x, dtype=F64):
    """x [R, C] -> (mean [C], M2 [C], T1 [C]) by the kernels' own tree of merges in `dtype` (fp64: the reference and the T1 of
    the bounds; fp32: a twin of the kernels).  Thread (blk, rl) owns rows (j * nblk + blk) * RPB + rl."""
    R, C = x.shape
    nblk, P = blocks(R), rpb(C)
    k = rows_per_thread(R, C)
    x = x.to(dtype)
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=x.device)
    xp = torch.cat([x, z(k * nblk * P - R, C)]).view(k, nblk, P, C)
    valid = (torch.arange(k * nblk * P, device=x.device) < R).to(dtype).view(k, nblk, P, 1)
    st = (z(nblk, P, 1), z(nblk, P, C), z(nblk, P, C), z(nblk, P, C))
    for j in range(k):                                                  # Welford: a merge with one element
        st = _merge(st, (valid[j], xp[j], z(nblk, P, C), z(nblk, P, C)))
    acc = tuple(t[:, 0] for t in st)
    for j in range(1, P):                                               # the row lanes of a workgroup, in order
        acc = _merge(acc, tuple(t[:, j] for t in st))
    G = -(-nblk // 64)
    part = tuple(torch.cat([t, z(G * 64 - nblk, t.shape[1])]).view(G, 64, t.shape[1]) for t in acc)
    lane = tuple(t[0] for t in part)
    for i in range(1, G):                                               # lane l: partials l, l + 64, ...
        lane = _merge(lane, tuple(t[i] for t in part))
    o = 32
    while o:                                                            # lane l takes lane l + o
        lane = _merge(tuple(t[:o] for t in lane), tuple(t[o:2 * o] for t in lane))
        o //= 2
    return lane[1][0], lane[2][0], lane[3][0]


# ---- the references ------------------------------------------------------------------------------------------------------
def stats(x):
    """-> mean [C], biased variance [C] in fp64."""
    x = x.to(F64)
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def running_update(running_mean, running_var, mean, var, R, momentum):
    """nn.BatchNorm2d's update: the batch mean and the UNBIASED variance enter with weight `momentum`."""
    m = float(momentum)
    return ((1 - m) * running_mean.to(F64) + m * mean.to(F64),
            (1 - m) * running_var.to(F64) + m * var.to(F64) * R / (R - 1))


def fwd(x, mean, rstd, gamma, beta, residual=None, relu=False):
    y = (x.to(F64) - mean.to(F64)) * (gamma.to(F64) * rstd.to(F64)) + beta.to(F64)
    if residual is not None:
        y = y + residual.to(F64)
    return y.clamp_min(0) if relu else y


def bwd(dy, x, y, mean, rstd, gamma, relu=False, frozen=False):
    """-> dx, g (= dres), dgamma, dbeta in fp64; the ReLU mask is y > 0 of the y it is given."""
    dy, x, mean, rstd, gamma = dy.to(F64), x.to(F64), mean.to(F64), rstd.to(F64), gamma.to(F64)
    g = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
    xh = (x - mean) * rstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    R = x.shape[0]
    dx = gamma * rstd * g if frozen else gamma * rstd * (g - dbeta / R - xh * dgamma / R)
    return dx, g, dgamma, dbeta


def pool_out(H):
    return (H - 1) // 2 + 1


def maxpool(x, last=False, admit_pad=False):
    """x [N, H, W, C] -> y [N, OH, OW, C], idx (kh * 3 + kw of the first maximum in row-major window order; padded positions
    skipped; a NaN counts as a maximum: ATen's rule).  Mutants: `last` keeps the last maximum, `admit_pad` lets a padded
    position take part with the value 0."""
    N, H, W, C = x.shape
    OH, OW = pool_out(H), pool_out(W)
    neg = float("-inf")
    best = torch.full((N, OH, OW, C), neg, dtype=x.dtype, device=x.device)
    idx = torch.full((N, OH, OW, C), -1, dtype=torch.int8, device=x.device)
    xp = F.pad(x, (0, 0, 1, 2, 1, 2), value=0.0 if admit_pad else neg)
    ok = F.pad(torch.ones(H, W, device=x.device), (1, 2, 1, 2), value=float(admit_pad)) > 0
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
            inside = ok[kh:kh + 2 * OH:2, kw:kw + 2 * OW:2][None, :, :, None]
            take = ((v >= best) if last else (v > best)) | torch.isnan(v) | (idx < 0)
            take = take & inside
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, kh * 3 + kw), idx)
    return best, idx


def maxpool_bwd(dy, idx, H, W):
    """dy, idx [N, OH, OW, C] -> dx [N, H, W, C] (fp64) and the sum of |terms| per element (the bound's scale)."""
    N, OH, OW, C = dy.shape
    dx = torch.zeros(N, H + 3, W + 3, C, dtype=F64, device=dy.device)
    sc = torch.zeros_like(dx)
    d = dy.to(F64)
    for kh in range(3):
        for kw in range(3):
            t = torch.where(idx == kh * 3 + kw, d, torch.zeros_like(d))
            dx[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += t
            sc[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += t.abs()
    return dx[:, 1:H + 1, 1:W + 1], sc[:, 1:H + 1, 1:W + 1]


def window_ties(x):
    """Number of pooling windows of x [N, H, W, C] in which the maximum is attained more than once."""
    y, _ = maxpool(x)
    N, H, W, C = x.shape
    OH, OW = y.shape[1:3]
    xp = F.pad(x, (0, 0, 1, 2, 1, 2), value=float("nan"))
    cnt = torch.zeros_like(y)
    for kh in range(3):
        for kw in range(3):
            cnt += (xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] == y).to(y.dtype)
    return int((cnt > 1).sum())


# ---- the bounds ----------------------------------------------------------------------------------------------------------
def stats_bounds(x, eps):
    """-> dict(mean, rstd, m2: absolute bounds [C]; and the fp64 mean, var, rstd, m2 they are about)."""
    x = x.to(F64)
    R, C = x.shape
    L = depth_stats(R, C)
    mean, m2, t1 = stats_walk(x)
    A, S = x.abs().amax(0), x.amax(0) - x.amin(0)
    dm = L * U * (A + 4 * S)
    dq = (2 * L + 6) * U * m2 + 4 * dm * t1 + R * dm * dm
    var = m2 / R
    relv = (dq / R) / (var + float(eps)) + 2 * U
    rstd = 1.0 / torch.sqrt(var + float(eps))
    return dict(mean=dm, m2=dq, rstd=(0.5 * relv * (1 + relv) + 5 * U) * rstd, ref_mean=mean, ref_var=var, ref_rstd=rstd, ref_m2=m2)


def running_bounds(running_mean, running_var, sb, R, momentum):
    """-> (reference running_mean, running_var; their absolute bounds) from stats_bounds()'s dict."""
    m = float(momentum)
    rm, rv = running_update(running_mean, running_var, sb["ref_mean"], sb["ref_var"], R, m)
    varu = sb["ref_m2"] / (R - 1)
    bm = abs(m) * sb["mean"] + 4 * U * (((1 - m) * running_mean.to(F64)).abs() + (m * sb["ref_mean"]).abs())
    bv = abs(m) * (sb["m2"] / (R - 1) + 2 * U * varu) + 4 * U * (((1 - m) * running_var.to(F64)).abs() + (m * varu).abs())
    return rm, rv, bm, bv


def fwd_bound(x, mean, rstd, gamma, beta, residual, relu, bf16_out):
    x, mean, rstd, gamma, beta = x.to(F64), mean.to(F64), rstd.to(F64), gamma.to(F64), beta.to(F64)
    ts = (x - mean) * (gamma * rstd)
    y0 = ts + beta
    b = 3 * U * ts.abs() + U * y0.abs()
    y = y0
    if residual is not None:
        y = y0 + residual.to(F64)
        b = b + U * y.abs()
    if bf16_out:
        b = b + bf_round(y.abs() + b)
    return b


def bwd_bounds(dy, x, y, mean, rstd, gamma, relu, frozen, bf16_out):
    """-> absolute bounds of dx [R, C], dgamma [C], dbeta [C]."""
    R, C = x.shape
    dx, g, dgamma, dbeta = bwd(dy, x, y, mean, rstd, gamma, relu, frozen)
    mean, rstd, gamma = mean.to(F64), rstd.to(F64), gamma.to(F64)
    xh = (x.to(F64) - mean) * rstd
    Ls = depth_sums(R, C)
    bb = Ls * U * g.abs().sum(0)
    bg = (Ls + 3) * U * (g * xh).abs().sum(0)
    a = (gamma * rstd).abs()
    if frozen:
        b = 2 * U * dx.abs()
    else:
        k1, k2 = dbeta / R, dgamma / R
        e1, e2 = bb / R + 2 * U * k1.abs(), bg / R + 2 * U * k2.abs()
        xk = (xh * k2).abs()
        b = a * (e1 + xh.abs() * e2 + 3 * U * xk + 2 * U * (g.abs() + k1.abs() + xk)) + 2 * U * dx.abs()
    if bf16_out:
        b = b + bf_round(dx.abs() + b)
    return b, bg, bb


def pool_bwd_bound(dx, scale, bf16_out):
    b = 3 * U * scale
    return b + bf_round(dx.abs() + b) if bf16_out else b


# ---- fp32 twins of the stages (CPU check of the bounds) and the mutants ----------------------------------------------------
def twin_stats(x, eps, naive=False):
    """fp32 -> mean, rstd, M2 the way the kernels form them (stats_walk in fp32); naive: E[x^2] - E[x]^2 in fp32."""
    x = x.float()
    R = x.shape[0]
    if naive:
        mean = x.sum(0) / R
        m2 = ((x * x).sum(0) / R - mean * mean) * R
    else:
        mean, m2, _ = stats_walk(x, torch.float32)
    return mean, 1.0 / torch.sqrt(m2 / R + torch.tensor(eps, dtype=torch.float32)), m2


def twin_running(running_mean, running_var, mean, m2, R, momentum, biased=False):
    m = torch.tensor(momentum, dtype=torch.float32)
    return ((1 - m) * running_mean.float() + m * mean.float(),
            (1 - m) * running_var.float() + m * (m2.float() / (R if biased else R - 1)))


def twin_fwd(x, mean, rstd, gamma, beta, residual, relu, out_dtype):
    y = (x.float() - mean) * (gamma * rstd) + beta
    if residual is not None:
        y = y + residual.float()
    return (y.clamp_min(0) if relu else y).to(out_dtype)


def twin_bwd(dy, x, y, mean, rstd, gamma, relu, frozen, out_dtype, mask_from_x=False):
    dy, x = dy.float(), x.float()
    g = torch.where((x if mask_from_x else y.float()) > 0, dy, torch.zeros_like(dy)) if relu else dy
    xh = (x - mean) * rstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    invR = torch.tensor(1.0 / x.shape[0], dtype=torch.float32)
    a = gamma * rstd
    dx = a * g if frozen else a * (g - dbeta * invR - xh * (dgamma * invR))
    return dx.to(out_dtype), g.to(out_dtype), dgamma, dbeta


# ---- a plain torch.nn restatement of STEVE's Res18Block (the public ResNet-18 structure, He et al. 2016) -------------------
class _Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        return self.relu(self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x))))) + idt)


class _Net(nn.Module):
    def __init__(self, img_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(img_channels, 64, 3, 1, 1)               # the replaced first convolution: 3x3 / 1, with bias
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = nn.Sequential(_Block(64, 64, 1), _Block(64, 64, 1))
        self.layer2 = nn.Sequential(_Block(64, 128, 2), _Block(128, 128, 1))
        self.layer3 = nn.Sequential(_Block(128, 256, 2), _Block(256, 256, 1))
        self.layer4 = nn.Sequential(_Block(256, 512, 2), _Block(512, 512, 1))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, 1000)


class Res18Restated(nn.Module):
    """conv1 -> bn1 -> ReLU -> MaxPool2d(3, 2, 1) -> layer1 -> ReLU -> ConvTranspose2d(64, d_model, 3, 2, 1, 1); layer2..4,
    avgpool and fc exist and never run.  `fenc` holds the first five children again, as the model's Sequential does."""

    def __init__(self, img_channels=3, d_model=192):
        super().__init__()
        self.res18 = _Net(img_channels)
        self.fenc = nn.Sequential(*list(self.res18.children())[:5])
        self.upconv = nn.ConvTranspose2d(64, d_model, 3, stride=2, padding=1, output_padding=1)

    def forward(self, x):
        return self.upconv(F.relu(self.fenc(x)))


N_STATE, N_FENC, N_PARAMS, N_LIVE, N_DEAD = 156, 31, 65, 18, 47
NUMEL_RES18, NUMEL_BLOCK_192 = 11681896, 11792680


# ---- the case table ------------------------------------------------------------------------------------------------------
ROWS_SMALL = (2, 63, 64, 65)
CHANNELS = (8, 64, 256)
FLAGS = [(relu, res, frozen) for relu in (False, True) for res in (False, True) for frozen in (False, True)]
POOL_HW = ((1, 1), (2, 2), (3, 5), (8, 8), (16, 16))
POOL_N = (1, 3)
EPS, MOMENTUM = 1e-5, 0.1


def first_rows_with_blocks_over(n, blocks_fn):
    """The smallest R whose reductions take more than n blocks (blocks_fn: focus_bn_blocks)."""
    R = 1
    while blocks_fn(R) <= n:
        R += 1
    return R


def first_rows_with_second_trip(C, blocks_fn):
    """The smallest R at which a thread of the row kernels walks its grid-stride loop twice: more than UNROLL rows per
    thread, R > UNROLL * blocks * RPB (blocks saturate, so the search ends)."""
    R = 1
    while R <= UNROLL * blocks_fn(R) * rpb(C):
        R = UNROLL * blocks_fn(R) * rpb(C) + 1
    return R


def inputs(R, C, dtype, seed, kind="randn", device="cpu"):
    """x, dy, residual [R, C] rounded to `dtype`, gamma (column 1 zero, signs mixed), beta, running buffers: fp32."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 31 + C)
    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == "offset":                                                # per-channel mean 100, std 0.1: the cancellation case
        x = 100.0 + 0.1 * rn(R, C)
    else:
        x = rn(R, C) * (0.5 + torch.rand(C, generator=g) * 2) + rn(C)
    t = dict(x=x.to(dtype), dy=rn(R, C).to(dtype), res=rn(R, C).to(dtype), gamma=rn(C), beta=rn(C),
             running_mean=rn(C), running_var=torch.rand(C, generator=g) + 0.5)
    if C > 1:
        t["gamma"][1] = 0.0
    return {k: v.to(device) for k, v in t.items()}
