"""focus_gemm by descriptor, in numpy (the checker of tests/test_gpu_gemm_desc.py; the product never imports this).

A descriptor addresses three flat buffers by ELEMENT strides (rs = row, cs = column) and a two-level batch
(bs0, bs1), as include/focus_amd.h states it:

    v = alpha * b_scale * A.B + bias            A [M,K], B [K,N], fp64 here, from the STORED operand values
    C = act(v) [* act'(aux)] + residual [+ C_old if accumulate]

view() / extent() turn (offset, rows, cols, strides, batch) into an as_strided window of a flat buffer; reference()
evaluates the formula through those windows and returns the whole C buffer as it must look after the call (so it
also states what must NOT change), the mask of the elements the call may write, and the same pair for aux.

CASES is the table the GPU test walks.  The expected routes (focus_gemm_kernel values) are written by hand from the
dispatch rules in csrc/gemm_mfma.hip (focus_gemm, focus_gemm_mfma_nt), gemm_mfma_ws.hip (dispatch_ws),
gemm_mfma_small.hip and gemm_mfma_tn.hip (the *_ok predicates); nothing here calls the library.
"""
import math

import numpy as np

F32, BF16, FP8_E4M3 = 0, 1, 2
EPI_NONE, EPI_GELU, EPI_RELU, EPI_TANH, EPI_DGELU, EPI_DRELU, EPI_DTANH = range(7)
GENERIC, NT, NT_WS, TN, NT_SMALL = 0, 1, 2, 3, 4          # enum focus_gemm_kernel
ROUTE_NAMES = {GENERIC: "GENERIC", NT: "NT", NT_WS: "NT_WS", TN: "TN", NT_SMALL: "NT_SMALL", None: "none"}

MARGIN = 256         # canary elements in front of and behind every C / aux window (one full tile row)


# ----------------------------------------------------------------------------------------------------------------
# windows
# ----------------------------------------------------------------------------------------------------------------
def extent(rows, cols, strides, b0, b1):
    """Last element touched by a [b0, b1, rows, cols] window, plus 1 (0 for an empty window).  Strides are >= 0."""
    if min(rows, cols, b0, b1) <= 0:
        return 0
    rs, cs, bs0, bs1 = strides
    return (rows - 1) * rs + (cols - 1) * cs + (b0 - 1) * bs0 + (b1 - 1) * bs1 + 1


def view(buf, off, rows, cols, strides, b0, b1):
    """as_strided view [b0, b1, rows, cols] of the flat buffer `buf` starting at element `off` (strides in elements)."""
    assert buf.ndim == 1
    assert off >= 0 and off + extent(rows, cols, strides, b0, b1) <= buf.shape[0], "window leaves the buffer"
    rs, cs, bs0, bs1 = strides
    it = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(b0, b1, rows, cols),
                                           strides=(bs0 * it, bs1 * it, rs * it, cs * it), writeable=True)


# ----------------------------------------------------------------------------------------------------------------
# activations (fp64)
# ----------------------------------------------------------------------------------------------------------------
_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(v):
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def dgelu(x):
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def activate(epi, v, x, xp=np, gelu_f=None, dgelu_f=None):
    """act(v) [* act'(x)] of enum focus_epilogue; x is the saved tensor of the derivative forms (else unused)."""
    gelu_f, dgelu_f = gelu_f or gelu, dgelu_f or dgelu
    if epi == EPI_NONE:
        return v
    if epi == EPI_GELU:
        return gelu_f(v)
    if epi == EPI_RELU:
        return xp.maximum(v, 0.0 * v)
    if epi == EPI_TANH:
        return xp.tanh(v)
    if epi == EPI_DGELU:
        return v * dgelu_f(x)
    if epi == EPI_DRELU:
        return v * (x > 0)
    if epi == EPI_DTANH:
        return v * (1.0 - x * x)
    raise ValueError(epi)


# ----------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------
def reference(case, bufs, parts=False):
    """-> (want_C, written_mask, want_aux, aux_mask): flat arrays as long as the C / aux buffers.

    bufs: flat numpy arrays of the STORED values: "A", "B" (an fp8 B already decoded, without b_scale), "C" (the
    pre-filled buffer), and where the case has them "bias" [N], "R" (residual), "X" (aux).  Everything is widened to
    float64, nothing is re-rounded.  want_aux / aux_mask are None when the case has no aux buffer (or uses it as the
    TN slab workspace).  parts=True appends a dict of the per-window terms (z, act, act' factor, mag_z = |alpha| sum|a||b| +
    |bias|, |residual|, |C_old|, ...) as [b0,b1,M,N] arrays:
    the GPU test builds its error magnitudes from them."""
    M, N, K = case["M"], case["N"], case["K"]
    b0, b1 = case["batch"]
    f8 = np.float64
    want_c = np.array(bufs["C"], dtype=f8)
    mask = np.zeros(want_c.shape, dtype=bool)
    has_x = case["aux"] and not case["tn_slab"]
    want_x = np.array(bufs["X"], dtype=f8) if has_x else None
    xmask = np.zeros(want_x.shape, dtype=bool) if has_x else None
    if min(M, N) <= 0:
        return (want_c, mask, want_x, xmask) + (({},) if parts else ())
    a = view(np.asarray(bufs["A"], dtype=f8), case["offA"], M, K, case["sA"], b0, b1)
    b = view(np.asarray(bufs["B"], dtype=f8), case["offB"], K, N, case["sB"], b0, b1)
    scale = f8(np.float32(case["alpha"])) * (f8(np.float32(case["b_scale"])) if case["fp8"] else 1.0)
    z = scale * np.matmul(a, b)
    bias = np.asarray(bufs["bias"], dtype=f8)[:N] if case["bias"] else np.zeros(N)
    z = z + bias
    cw = view(want_c, case["offC"], M, N, case["sC"], b0, b1)
    c_old = cw.copy()
    x = view(want_x, case["offX"], M, N, case["sC"], b0, b1).copy() if has_x else None
    act = activate(case["epi"], z, x)
    res = view(np.asarray(bufs["R"], dtype=f8), case["offR"], M, N, case["sC"], b0, b1) if case["residual"] else 0.0 * z
    out = act + res + (c_old if case["accumulate"] else 0.0)
    cw[...] = out
    view(mask, case["offC"], M, N, case["sC"], b0, b1)[...] = True
    if has_x and case["epi"] == EPI_GELU:
        view(want_x, case["offX"], M, N, case["sC"], b0, b1)[...] = z
        view(xmask, case["offX"], M, N, case["sC"], b0, b1)[...] = True
    if not parts:
        return want_c, mask, want_x, xmask
    # the dot-product magnitude only where a bound uses it (fp32 C)
    mag_z = abs(scale) * np.matmul(np.abs(a), np.abs(b)) + np.abs(bias) if case.get("dtype_c", F32) == F32 else None
    fac = activate(case["epi"], np.ones_like(z), x) if case["epi"] >= EPI_DGELU else np.ones_like(z)      # act'(aux)
    p = dict(z=z, act=act, mag_z=mag_z, res=np.abs(res), c_old=np.abs(c_old) if case["accumulate"] else 0.0 * z, x=x, out=out,
             fac=fac)
    return want_c, mask, want_x, xmask, p


def reference_torch(case, bufs, parts=False):
    """reference() with torch, in float64 on the device the buffers live on (the product-size rows).  Same contract,
    torch tensors instead of arrays; the written masks come from window_masks() (numpy)."""
    import torch
    M, N, K = case["M"], case["N"], case["K"]
    b0, b1 = case["batch"]

    def win(t, off, rows, cols, s):
        assert off + extent(rows, cols, s, b0, b1) <= t.numel(), "window leaves the buffer"
        return torch.as_strided(t, (b0, b1, rows, cols), (s[2], s[3], s[0], s[1]), off)

    has_x = case["aux"] and not case["tn_slab"]
    want_c = bufs["C"].double().clone()
    want_x = bufs["X"].double().clone() if has_x else None
    if min(M, N) <= 0:
        return (want_c, None, want_x, None) + (({},) if parts else ())
    a = win(bufs["A"], case["offA"], M, K, case["sA"]).double()
    b = win(bufs["B"], case["offB"], K, N, case["sB"]).double()
    scale = float(np.float32(case["alpha"])) * (float(np.float32(case["b_scale"])) if case["fp8"] else 1.0)
    bias = bufs["bias"][:N].double() if case["bias"] else torch.zeros(N, dtype=torch.float64, device=want_c.device)
    z = scale * torch.matmul(a, b) + bias
    cw = win(want_c, case["offC"], M, N, case["sC"])
    c_old = cw.clone()
    x = win(want_x, case["offX"], M, N, case["sC"]).clone() if has_x else None
    g = lambda v: 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    dg = lambda v: 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    act = activate(case["epi"], z, x, xp=torch, gelu_f=g, dgelu_f=dg)
    res = win(bufs["R"], case["offR"], M, N, case["sC"]).double() if case["residual"] else torch.zeros_like(z)
    out = act + res + (c_old if case["accumulate"] else 0.0)
    cw.copy_(out)
    if has_x and case["epi"] == EPI_GELU:
        win(want_x, case["offX"], M, N, case["sC"]).copy_(z)
    if not parts:
        return want_c, None, want_x, None
    # the dot-product magnitude only where a bound uses it (fp32 C): it doubles the fp64 work of the large rows
    mag_z = abs(scale) * torch.matmul(a.abs(), b.abs()) + bias.abs() if case["dtype_c"] == F32 else None
    fac = activate(case["epi"], torch.ones_like(z), x, xp=torch, gelu_f=g, dgelu_f=dg) if case["epi"] >= EPI_DGELU \
        else torch.ones_like(z)
    p = dict(z=z, act=act, mag_z=mag_z, res=res.abs(), c_old=c_old.abs() if case["accumulate"] else torch.zeros_like(z),
             x=x, out=out, fac=fac)
    return want_c, None, want_x, None, p


def window_masks(case):
    """(written_mask of C, aux_mask or None) from the descriptor alone (no operand values)."""
    M, N = case["M"], case["N"]
    b0, b1 = case["batch"]
    mask = np.zeros(case["lenC"], dtype=bool)
    if min(M, N) > 0:
        view(mask, case["offC"], M, N, case["sC"], b0, b1)[...] = True
    if not case["aux"] or case["tn_slab"]:
        return mask, None
    xmask = np.zeros(case["lenX"], dtype=bool)
    if case["epi"] == EPI_GELU and min(M, N) > 0:
        view(xmask, case["offX"], M, N, case["sC"], b0, b1)[...] = True
    return mask, xmask


def prefill(n):
    """The recognisable pre-fill of C and aux: finite, non-zero almost everywhere, exact in bf16 (|k| <= 125 over 64),
    different at neighbouring and at tile-periodic positions (period 251 is prime)."""
    i = np.arange(n, dtype=np.int64)
    return (((i * 7) % 251 - 125) / 64.0).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------
CASES = []


def _case(name, M, N, K, sA, sB, sC, route, batch=(1, 1), ab=BF16, c=BF16, offA=0, offB=0, offC=MARGIN, offR=MARGIN,
          offX=MARGIN, bias=False, residual=False, aux=False, alpha=1.0, accumulate=False, epi=EPI_NONE, fp8=False,
          b_scale=1.0, tn_slab=False, tile=0, atomic=False, col_sliced=False, padA=8, padB=16):
    b0, b1 = batch
    if epi >= EPI_DGELU:
        aux = True
    flops = 2.0 * max(M, 0) * max(N, 0) * max(K, 0) * b0 * b1
    d = dict(name=name, M=M, N=N, K=K, batch=batch, sA=tuple(sA), sB=tuple(sB), sC=tuple(sC), route=route,
             dtype_ab=ab, dtype_c=c, offA=offA, offB=offB, offC=offC, offR=offR, offX=offX,
             bias=bias, residual=residual, aux=aux or tn_slab, alpha=alpha, accumulate=accumulate, epi=epi,
             fp8=fp8, b_scale=b_scale, tn_slab=tn_slab, tile=tile, atomic=atomic, col_sliced=col_sliced,
             lenA=offA + extent(M, K, sA, b0, b1) + padA,
             lenB=offB + extent(K, N, sB, b0, b1) + padB,
             lenC=offC + extent(M, N, sC, b0, b1) + MARGIN,
             lenR=offR + extent(M, N, sC, b0, b1) + MARGIN,
             lenX=offX + extent(M, N, sC, b0, b1) + MARGIN,      # slab mode: the workspace is sized by the library's own query
             lenBias=max(N, 1),
             # the fp64 reference of anything above ~0.3 GFLOP runs with torch on the device
             ref="torch" if flops > 3e8 else "numpy")
    assert name not in [k["name"] for k in CASES], name
    CASES.append(d)
    return d


def _nt(M, N, K, lda=None, ldb=None, ldc=None):
    """strides of the nn.Linear layout: A [M,K] rows, B given as [N,K] rows, C [M,N] rows."""
    return ((lda or K, 1, 0, 0), (1, ldb or K, 0, 0), (ldc or N, 1, 0, 0))


# ---- trajectory time step, dq2 (_TrajTime2BlockFn.backward): g [heads, R, C] . wk[h]^T -> a 64-column stripe of a shared row.
# The product writes rsC = C; here the row is two stripes wider (one unwritten stripe on each side: the only thing between
# a tile and its neighbour's stripe is the column tail mask).  Route: N = 64, no epilogue:
#   the narrow 256x64 instance needs M >= 2048 and ceil(M/256) * heads >= 192; below that N < 256 and
#   ceil(M/256) * ceil(N/128) < 192 leave the uniform kernel; M <= 1024 takes the small kernel first.
def _dq2(name, R, Cc, route, **kw):
    heads, d = Cc // 64, 64
    ldc = Cc + 2 * d
    return _case(name, R, d, Cc, (Cc, 1, 0, R * Cc), (1, Cc, 0, d * Cc), (ldc, 1, 0, d), route, batch=(1, heads),
                 offC=MARGIN + d, offR=MARGIN + d, offX=MARGIN + d, col_sliced=True, **kw)


_dq2("dq2 R12544 C768", 12544, 768, NT_WS)      # 49 * 12 = 588 row tiles: the product shape
_dq2("dq2 R4100 C768", 4100, 768, NT_WS)        # 17 * 12 = 204 >= 192
_dq2("dq2 R1000 C768", 1000, 768, NT_SMALL)
_dq2("dq2 R37 C768", 37, 768, NT_SMALL)
_dq2("dq2 R12544 C192", 12544, 192, NT)         # 49 * 3 = 147 < 192, t256 = 49 < 192
_dq2("dq2 R4100 C192", 4100, 192, NT)           # 17 * 3 = 51
_dq2("dq2 R1000 C192", 1000, 192, NT_SMALL)
_dq2("dq2 R37 C192", 37, 192, NT_SMALL)
# the same with bias, residual and every epilogue (aux column-sliced like C).  An activation takes the descriptor off
# the narrow instance (it is built for EPI_NONE only) and t256 = ceil(M/256) * 1 < 192 -> uniform kernel, LDS epilogue;
# EPI_NONE with bias and residual stays on the narrow instance (its condition looks at the epilogue alone).
for _e in range(7):
    _dq2("dq2 R12544 C768 epi%d" % _e, 12544, 768, NT_WS if _e == EPI_NONE else NT, bias=True, residual=True,
         aux=_e in (EPI_GELU, EPI_DGELU, EPI_DRELU, EPI_DTANH), epi=_e)
    _dq2("dq2 R4100 C768 epi%d" % _e, 4100, 768, NT_WS if _e == EPI_NONE else NT, bias=True, residual=True,
         aux=_e in (EPI_GELU, EPI_DGELU, EPI_DRELU, EPI_DTANH), epi=_e, alpha=0.5 if _e & 1 else 1.0)


# ---- unfused small attention (_SmallAttnFn), two-level batch (B, heads).  q/k/v/out rows are C = heads*d wide (here two
# head widths wider for the column-sliced outputs), att is [B, heads, n, m].
def _attn(d, n, m, tag, qk_route):
    B, heads = 2, 3
    Cc = heads * d
    ldo = Cc + 2 * d
    sq, sk = (Cc, 1, n * Cc, d), (Cc, 1, m * Cc, d)
    so_n, so_m = (ldo, 1, n * ldo, d), (ldo, 1, m * ldo, d)
    sa, sat = (m, 1, heads * n * m, n * m), (1, m, heads * n * m, n * m)
    kw = dict(batch=(B, heads))
    off = dict(offC=MARGIN + d, offR=MARGIN + d, offX=MARGIN + d, col_sliced=True)
    # K = d: 64 -> MFMA layout (few rows: small kernel while rsC % 4 == 0, else the uniform kernel's direct epilogue);
    # 48 is not a multiple of 64 -> generic
    _case("attn%s q.kT" % tag, n, m, d, sq, (1, Cc, m * Cc, d), sa, qk_route, alpha=d ** -0.5, **kw)
    # csB == 1 (v read row-major) and rsA != 1: neither MFMA form -> generic, in bf16
    _case("attn%s att.v" % tag, n, d, m, sa, (Cc, 1, m * Cc, d), so_n, GENERIC, **kw, **off)
    _case("attn%s datt=dout.vT" % tag, n, m, d, sq, (1, Cc, m * Cc, d), sa, qk_route, **kw)
    # transposed A (rsA == 1) with a bf16 C: the TN form wants fp32 out -> generic
    _case("attn%s dv=attT.dout" % tag, m, d, n, sat, sq, so_m, GENERIC, **kw, **off)
    _case("attn%s dq=datt.k" % tag, n, d, m, sa, sk, so_n, GENERIC, **kw, **off)
    _case("attn%s dk=dattT.q" % tag, m, d, n, sat, sq, so_m, GENERIC, **kw, **off)


_attn(64, 50, 36, " d64", NT_SMALL)
_attn(48, 50, 36, " d48", GENERIC)
# m = 37: att rows are not 8-byte multiples -> not the small kernel (rsC % 4), not the LDS epilogue (rsC % 8): uniform
# kernel, direct bf16 epilogue, scalar stores
_case("attn d64 q.kT m37", 50, 37, 64, (192, 1, 50 * 192, 64), (1, 192, 37 * 192, 64), (37, 1, 3 * 50 * 37, 50 * 37), NT,
      batch=(2, 3), alpha=0.125)

# ---- GRU (_GruCellFn): batch (1,2) over [x | h], the batch stride of A is the distance between two operands placed
# separately in one buffer; backward adds a batched residual.  R = 352 rows -> small kernel.
_R, _D, _G = 352, 192, 576
_case("gru fwd", _R, _G, _D, (_D, 1, 0, _R * _D + 4104), (1, _D, 0, _G * _D), (_G, 1, 0, _R * _G), NT_SMALL, batch=(1, 2),
      offA=24, aux=True)                                    # an aux pointer without an activation is ignored
_case("gru bwd", _R, _D, _G, (_G, 1, 0, _R * _G), (1, _G, 0, _D * _G), (_D, 1, 0, _R * _D), NT_SMALL, batch=(1, 2),
      residual=True)

# ---- NT with offsets, row-padded A (rsA > K) and C (rsC > N)
# 8200 x 768: 128-row tiles: 65*3 = 195 (>= 128, one round, cost 168; 160: 156 tiles cost 200; 192: 129 tiles cost 232)
# and tw = 195 >= 192 -> wave-specialised 128x256
_case("nt offsets ws", 8200, 768, 256, (264, 1, 0, 0), (1, 272, 0, 0), (776, 1, 0, 0), NT_WS, offA=16, offB=8, offC=MARGIN + 8,
      offR=MARGIN + 16, offX=MARGIN + 24, bias=True, residual=True, aux=True, epi=EPI_GELU)
# 1100 x 136: more than 1024 rows, 9*2 tiles: uniform kernel
_case("nt offsets uniform", 1100, 136, 128, (136, 1, 0, 0), (1, 144, 0, 0), (152, 1, 0, 0), NT, offA=8, offB=24, offC=MARGIN + 16,
      offR=MARGIN + 8, offX=MARGIN + 8, bias=True, residual=True, aux=True, epi=EPI_TANH)      # aux given, must stay untouched
_case("nt offsets small", 300, 200, 192, (200, 1, 0, 0), (1, 208, 0, 0), (208, 1, 0, 0), NT_SMALL, offA=8, offB=16,
      offC=MARGIN + 8, offR=MARGIN + 24, offX=MARGIN + 16, bias=True, residual=True, epi=EPI_DGELU, alpha=-0.75)

# ---- NT, bf16 in, fp32 C, no split (K < 1024); accumulate keeps a product off the small kernel
_case("nt f32 M1100", 1100, 200, 512, *_nt(1100, 200, 512), NT, c=F32, bias=True, residual=True)
_case("nt f32 M1100 acc", 1100, 200, 512, *_nt(1100, 200, 512, ldc=204), NT, c=F32, accumulate=True, alpha=0.5)
_case("nt f32 M300", 300, 200, 512, *_nt(300, 200, 512), NT_SMALL, c=F32, bias=True, residual=True)
_case("nt f32 M300 acc", 300, 200, 512, *_nt(300, 200, 512), NT, c=F32, accumulate=True)
_case("small f32 gelu", 300, 72, 192, *_nt(300, 72, 192), NT_SMALL, c=F32, bias=True, aux=True, epi=EPI_GELU)
_case("small f32 dtanh", 300, 72, 192, *_nt(300, 72, 192), NT_SMALL, c=F32, residual=True, epi=EPI_DTANH, alpha=0.5)
# bf16 C whose rows are not 16-byte multiples: direct epilogue of the uniform kernel (rsC = 102 also fails the small
# kernel's rsC % 4)
_case("nt bf16 rsC100 M1100", 1100, 100, 128, *_nt(1100, 100, 128), NT, alpha=0.5)
_case("nt bf16 rsC102 M300", 300, 100, 128, *_nt(300, 100, 128, ldc=102), NT)

# ---- split-K: accumulate, fp32 C, no bias/residual/epilogue, batch 1, t128 < 256, K >= 1024 (atomics: not bitwise
# reproducible)
_case("splitk K1024", 333, 200, 1024, *_nt(333, 200, 1024), NT, c=F32, accumulate=True, atomic=True)
_case("splitk K4096", 129, 97, 4096, *_nt(129, 97, 4096), NT, c=F32, accumulate=True, atomic=True, alpha=0.5)
_case("splitk K12608", 333, 200, 12608, *_nt(333, 200, 12608, ldc=208), NT, c=F32, accumulate=True, atomic=True)


# ---- TN (weight-gradient form): A[i,m] = P[m,i] (rsA = 1, csA = ldp), B[m,j] = Q[m,j] (csB = 1), fp32 C.
def _tn(name, M, N, K, slab, ldp=None, ldq=None, ldc=None, **kw):
    return _case(name, M, N, K, (1, ldp or M, 0, 0), (ldq or N, 1, 0, 0), (ldc or N, 1, 0, 0), TN, c=F32,
                 tn_slab=slab, accumulate=not slab, atomic=not slab, **kw)


_tn("tn atomic 136x8 K2055", 136, 8, 2055, False, alpha=0.5)
_tn("tn atomic 768x768 K4104", 768, 768, 4104, False, ldp=776)           # large output, long reduction: wave-specialised TN
_tn("tn atomic 8x136 K1", 8, 136, 1, False, ldc=140)
_tn("tn slab 8x136 K4104", 8, 136, 4104, True, ldc=144, alpha=0.5)
_tn("tn slab 768x136 K2055", 768, 136, 2055, True, ldc=152, ldq=144)
_tn("tn slab 136x136 K1", 136, 136, 1, True)                             # one split, dense C: the slab is C itself
_tn("tn slab 136x136 K1 rsC", 136, 136, 1, True, ldc=140)
_tn("tn slab 8x8 K2055", 8, 8, 2055, True, alpha=0.5)
# batched slab mode, the dWk form of _TrajTime2BlockFn: q2 [R, C] (head stripe) ^T . g [heads, R, C] -> dw [heads*d, C]
for _Rr in (4100, 37):
    _case("tn batched dWk R%d" % _Rr, 64, 192, _Rr, (1, 192, 0, 64), (192, 1, 0, _Rr * 192), (192, 1, 0, 64 * 192), TN,
          batch=(1, 3), c=F32, tn_slab=True)

# ---- generic kernel, fp32 everywhere: NN / NT / TN forms, two-level batch, transposed C, all epilogues
_M, _N, _K = 70, 90, 50
_NN = ((_K, 1, 3 * _M * _K, _M * _K), (_N, 1, 3 * _K * _N, _K * _N))
_NTf = ((_K + 2, 1, 0, _M * (_K + 2)), (1, _K, 0, _N * _K))
_TNf = ((1, _M, 0, _K * _M), (_N + 1, 1, 0, _K * (_N + 1)))
_Cd = (_N, 1, 3 * _M * _N, _M * _N)
_Ct = (1, _M, 3 * _M * _N, _M * _N)          # C^T stored: csC = M
_case("generic f32 NN epi0", _M, _N, _K, *_NN, _Cd, GENERIC, batch=(2, 3), ab=F32, c=F32, alpha=-1.5, accumulate=True,
      bias=True, residual=True)
_case("generic f32 NT epi1 Ct", _M, _N, _K, *_NTf, _Ct, GENERIC, batch=(1, 3), ab=F32, c=F32, bias=True, aux=True, epi=EPI_GELU)
_case("generic f32 TN epi2", _M, _N, _K, *_TNf, _Cd, GENERIC, batch=(1, 3), ab=F32, c=F32, bias=True, aux=True, epi=EPI_RELU, alpha=-1.5)
_case("generic f32 NN epi3", _M, _N, _K, *_NN, _Cd, GENERIC, batch=(2, 3), ab=F32, c=F32, residual=True, epi=EPI_TANH)
_case("generic f32 NT epi4 Ct", _M, _N, _K, *_NTf, _Ct, GENERIC, batch=(1, 3), ab=F32, c=F32, epi=EPI_DGELU, alpha=-1.5)
_case("generic f32 TN epi5", _M, _N, _K, *_TNf, _Cd, GENERIC, batch=(1, 3), ab=F32, c=F32, residual=True, epi=EPI_DRELU)
_case("generic f32 NN epi6 acc", _M, _N, _K, *_NN, _Cd, GENERIC, batch=(2, 3), ab=F32, c=F32, accumulate=True, epi=EPI_DTANH)
# the mm_nn form as ops.mm_nn issues it (one dense product, row-major B)
_case("generic f32 mm_nn", 130, 67, 33, (33, 1, 0, 0), (67, 1, 0, 0), (67, 1, 0, 0), GENERIC, ab=F32, c=F32)
# mixed storage / layouts the MFMA kernels refuse
_case("generic bf16->f32 K100", 150, 72, 100, *_nt(150, 72, 100, lda=104, ldb=104), GENERIC, c=F32, bias=True)
_case("generic f32->bf16", 150, 72, 100, *_nt(150, 72, 100), GENERIC, ab=F32, bias=True, residual=True, epi=EPI_RELU)
_case("generic bf16 K100", 150, 72, 100, *_nt(150, 72, 100, lda=104, ldb=104), GENERIC, bias=True, aux=True, epi=EPI_GELU)
_case("generic bf16 A+2B", 150, 72, 64, *_nt(150, 72, 64, lda=72), GENERIC, offA=1, residual=True)    # A 2 bytes off 16-byte alignment

# ---- e4m3 weights (B holds codes, 1 byte per element), bf16 activations: always the wave-specialised kernel
_case("fp8w batch2 gelu", 300, 264, 128, (136, 1, 0, 300 * 136), (1, 128, 0, 264 * 128), (272, 1, 0, 300 * 272), NT_WS,
      batch=(1, 2), fp8=True, b_scale=0.37, alpha=0.5, bias=True, aux=True, epi=EPI_GELU)
_case("fp8w N136", 700, 136, 192, (200, 1, 0, 0), (1, 192, 0, 0), (144, 1, 0, 0), NT_WS, fp8=True, b_scale=1.75,
      residual=True)

# ---- degenerate sizes: K == 0 gives C = epi(bias) + residual (generic kernel: no MFMA form takes K <= 0);
# M == 0 / N == 0 return FOCUS_OK before any dispatch and leave C alone
_case("K0 bf16 gelu", 150, 72, 0, (64, 1, 0, 0), (1, 64, 0, 0), (72, 1, 0, 0), GENERIC, bias=True, residual=True, aux=True,
      epi=EPI_GELU)
_case("K0 f32 acc", 70, 90, 0, (8, 1, 0, 0), (1, 8, 0, 0), (90, 1, 0, 0), GENERIC, ab=F32, c=F32, bias=True, accumulate=True)
_case("M0", 0, 72, 64, *_nt(1, 72, 64), None, bias=True)
_case("N0", 150, 0, 64, *_nt(150, 8, 64), None, c=F32, accumulate=True)

# ---- the five wave-specialised instances.  N >= 256, batch 1: the tile height is 128, 160 or 192 by modelled cost (rounds of
# 256 workgroups x (height + 40)) among heights with >= 128 tiles; 128 also needs ceil(M/128) * ceil(N/256) >= 192.
# Forced heights (focus_gemm_tile_override), M = -1, 0, +1 around a multiple of the height, N ragged against 256:
_EPIS = [dict(), dict(bias=True, epi=EPI_RELU), dict(bias=True, residual=True, aux=True, epi=EPI_GELU),
         dict(epi=EPI_DGELU, alpha=0.5), dict(residual=True, epi=EPI_TANH), dict(epi=EPI_DRELU, bias=True),
         dict(epi=EPI_DTANH, residual=True), dict(bias=True, residual=True), dict(alpha=-0.5)]
_i = 0
for _h, _Nn, _mult, _Kk in ((128, 776, 48, 128), (160, 520, 43, 64), (192, 264, 64, 192)):
    for _dm in (-1, 0, 1):
        _Mm = _h * _mult + _dm            # tiles: 48*4 = 192, 43*3 = 129, 64*2 = 128 (and one more row tile for +1)
        _case("ws tile%d M%d N%d" % (_h, _Mm, _Nn), _Mm, _Nn, _Kk, *_nt(_Mm, _Nn, _Kk), NT_WS, tile=_h, **_EPIS[_i])
        _i += 1
# automatic choice: 10000 x 776: 128 -> 316 tiles, 2 rounds, cost 336; 160 -> 252 tiles, cost 200; 192 -> 212, cost 232
_case("ws auto 160", 10000, 776, 64, *_nt(10000, 776, 64), NT_WS, bias=True)
# 12001 x 776: 128 -> 376 tiles (336); 160 -> 304 tiles, 2 rounds (400); 192 -> 252 tiles (232)
_case("ws auto 192", 12001, 776, 64, *_nt(12001, 776, 64), NT_WS, residual=True)
# batch (1,2) skips the cost branch: N >= 256 and ceil(M/128) * ceil(N/256) = 49*4 >= 192 -> 128x256
_case("ws batch2 128x256", 6145, 776, 64, (64, 1, 0, 6145 * 64), (1, 64, 0, 776 * 64), (776, 1, 0, 6145 * 776), NT_WS,
      batch=(1, 2), bias=True, epi=EPI_RELU)
# 256x128: N < 256, ceil(M/256) * ceil(N/128) = 96*2 >= 192
_case("ws 256x128", 24500, 136, 64, *_nt(24500, 136, 64), NT_WS, bias=True, residual=True, aux=True, epi=EPI_GELU)
_case("ws 256x128 batch2", 24500, 136, 64, (64, 1, 0, 24500 * 64), (1, 64, 0, 136 * 64), (136, 1, 0, 24500 * 136), NT_WS,
      batch=(1, 2), residual=True)
# refusals, just under each threshold: the uniform kernel computes the same values
_case("ws refuse tiles lt 128", 8064, 264, 64, *_nt(8064, 264, 64), NT, bias=True)        # 63*2 = 126 tiles of 128 rows; t256 = 32*3
_case("ws refuse tw lt 192", 6016, 776, 64, *_nt(6016, 776, 64), NT, residual=True)       # 47*4 = 188 (cost picks 128); t256 = 24*7 = 168
_case("ws refuse t256 lt 192", 24320, 136, 64, *_nt(24320, 136, 64), NT, bias=True, epi=EPI_RELU)   # 95*2 = 190

BY_NAME = {c["name"]: c for c in CASES}
