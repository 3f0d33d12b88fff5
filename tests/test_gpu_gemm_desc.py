"""focus_gemm by descriptor: every kernel family behind the one entry point, reached through ops.gemm with the
descriptors the product sends (head-batched column-sliced C, two-level batches, pointer-difference batch strides,
slab-mode TN, alpha / accumulate / split-K, degenerate sizes), each against the fp64 reference of tests/gemm_ref.py:

  route   focus_gemm_last_kernel() equals the route written by hand in gemm_ref.CASES;
  values  inside the written window, at the limits tests/test_gpu_kernels.py derives (see _check_values);
  window  every element of C and aux outside the window keeps the bits of its pre-fill; operands are untouched;
  repeat  a second launch gives the same bits wherever no atomics are involved.

The table itself (bounds of every window, preconditions of every route) is checked without a GPU in
tests/test_gemm_desc_cpu.py."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import gemm_ref as gr
from test_gpu_kernels import GEMM_SWITCHES as SWITCHES
from test_gpu_kernels import Check, U, bf, dgelu64
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

# SWITCHES: process-wide dispatch switches (read once by the library): with one of them set the route is not asserted
TDT = {gr.F32: torch.float32, gr.BF16: torch.bfloat16}
ONE, TWO = 1.01 * U, 2.02 * U
# fp32 activations (focus_common.h): erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, evaluated with one rcp, one exp2
# (1 ulp each) and five fma: |d erf| <= 1.5e-7 + 4 * 2^-24 = 3.9e-7, so |d gelu| = |z| / 2 * |d erf| + 2 roundings of the
# product <= (1.95e-7 + 1.2e-7) |z| = 3.2e-7 |z|;  gelu' = cdf + z pdf: 1.95e-7 + 3 roundings of a term <= 0.25: < 3e-7;
# tanhf (ocml, 2 ulp): 2.4e-7 |tanh z| <= 2.4e-7 |z|;  1 - x*x: 2^-24 (1 + 2 x^2).  One constant covers them all:
#   |d (act(z) act'(x))| <= EPS_ACT |z| (1 + x^2)      at exact z
EPS_ACT = 4e-7


def _win(t, off, case):
    b0, b1 = case["batch"]
    s = case["sC"]
    assert off + gr.extent(case["M"], case["N"], s, b0, b1) <= t.numel()
    return torch.as_strided(t, (b0, b1, case["M"], case["N"]), (s[2], s[3], s[0], s[1]), off)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.uint8 if t.dtype == torch.uint8 else torch.int32)


def _prefill(n, d):
    """gemm_ref.prefill evaluated on the device (the same integers, exact in fp32), checked against it on a prefix."""
    i = torch.arange(n, device=d, dtype=torch.int64)
    p = ((i * 7) % 251 - 125).float() / 64.0
    assert np.array_equal(p[:4096].cpu().numpy(), gr.prefill(min(n, 4096)))
    return p


def _build(case, d):
    g = torch.Generator(device=d).manual_seed(zlib.crc32(case["name"].encode()))
    ab, cdt = TDT[case["dtype_ab"]], TDT[case["dtype_c"]]
    t = {}
    t["A"] = bf(torch.randn(case["lenA"], device=d, generator=g)).to(ab)
    if case["fp8"]:
        from oracle import fp8
        # exponent field <= 7: |value| < 2, never the NaN code
        t["B"] = (torch.randint(0, 256, (case["lenB"],), device=d, generator=g, dtype=torch.int32) & 0xBF).to(torch.uint8)
        table = torch.from_numpy(np.asarray(fp8.decode_table(), dtype=np.float32)).to(d)
        t["Bval"] = table[t["B"].long()]
        t["b_scale"] = torch.tensor([case["b_scale"]], device=d, dtype=torch.float32)
    else:
        t["B"] = bf(torch.randn(case["lenB"], device=d, generator=g) * max(case["K"], 1) ** -0.5).to(ab)
        t["Bval"] = t["B"]
    t["bias"] = torch.randn(case["lenBias"], device=d, generator=g)
    t["R"] = bf(torch.randn(case["lenR"], device=d, generator=g)).to(cdt)
    t["C"] = _prefill(case["lenC"], d).to(cdt)
    t["X"] = _prefill(case["lenX"] + 13, d)[13:].clone().to(cdt)
    if case["tn_slab"]:
        from focus_amd import _lib
        L = _lib.lib()
        b1 = case["batch"][1]
        nb = (L.focus_gemm_tn_batched_workspace_bytes(case["M"], case["N"], case["K"], b1) if b1 > 1
              else L.focus_gemm_tn_workspace_bytes(case["M"], case["N"], case["K"]))
        t["ws"] = torch.zeros(nb // 4 + 4, device=d, dtype=torch.float32)
    return t


def _launch(case, t):
    from focus_amd import _lib, ops
    L = _lib.lib()
    aux = (t["ws"], 0) if case["tn_slab"] else (t["X"], case["offX"]) if case["aux"] else None
    if case["tile"]:
        assert L.focus_gemm_tile_override(case["tile"]) == 0
    try:
        ops.gemm(case["M"], case["N"], case["K"], (t["A"], case["offA"]), case["sA"], (t["B"], case["offB"]), case["sB"],
                 (t["C"], case["offC"]), case["sC"], batch=case["batch"], bias=t["bias"] if case["bias"] else None,
                 residual=(t["R"], case["offR"]) if case["residual"] else None, aux=aux, alpha=case["alpha"],
                 accumulate=case["accumulate"], epilogue=case["epi"], b_scale=t["b_scale"] if case["fp8"] else None)
        route = L.focus_gemm_last_kernel()
    finally:
        if case["tile"]:
            L.focus_gemm_tile_override(0)
    torch.cuda.synchronize()
    return route


def _reference(case, t):
    """fp64 reference where it is computed: numpy on the host, or torch on the device for the large rows."""
    if case["ref"] == "torch":
        bufs = dict(A=t["A"], B=t["Bval"], C=t["C0"], X=t["X0"], R=t["R"], bias=t["bias"])
        want_c, _, want_x, _, p = gr.reference_torch(case, bufs, parts=True)
        return want_c, want_x, p
    bufs = {k: v.float().cpu().numpy() for k, v in dict(A=t["A"], B=t["Bval"], C=t["C0"], X=t["X0"], R=t["R"], bias=t["bias"]).items()}
    want_c, mask, want_x, xmask, p = gr.reference(case, bufs, parts=True)
    m2, xm2 = gr.window_masks(case)
    assert np.array_equal(mask, m2) and (xmask is None or np.array_equal(xmask, xm2))
    tt = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    return tt(want_c), tt(want_x), {k: tt(v) for k, v in p.items()}


def _check_values(ck, case, tag, got_c, got_x, want_c, want_x, p):
    """Limits, per output type and epilogue (U = 2^-8, the bf16 unit roundoff):

    bf16 C   one output rounding (plain, alpha, bias, the ReLU masks)                          1.01 U
             forms that touch the rounded z again (tanh, x gelu', x (1 - y^2), + residual)     2.02 U, mag = |act part|
             GELU: gelu(round z) rounded: (|z gelu'| + |gelu|) U <= 2.3 U |gelu|               3 U
             GELU + residual: the 2.3 above bounds |z gelu'(z)| by |gelu(z)|, which holds for z > 0 only (at z = -2,
             |z gelu'| = 0.17 against |gelu| = 0.045) and is rescued there by the floor; next to a residual the sum can
             be small where that term is not, so the first-order bound is used as it stands: rounding z moves gelu by
             U |z gelu'(z)|, the sum is rounded once:                          1.01 U, mag = |z gelu'(z)| + |C|
    fp32 C   no output rounding: gamma = (K + 4) 2^-24 against mag = |alpha| sum|a||b| + |bias| + |residual| + |C_old|
             (the dot-product bound: any summation order, split-K and slab partial sums included), floor 0.
             With an activation the bound holds for z; it passes through |act'| <= 1.13 (or the act'(aux) factor itself
             for the derivative forms), the activation adds EPS_ACT |z| (1 + aux^2) (derived at EPS_ACT above) and the
             remaining additions at most 3 x 2^-24 <= gamma of the terms they sum:
                 mag = G mag_z + |act| + |residual| + |C_old| + (EPS_ACT / gamma) |z| (1 + aux^2)

    Observed on an MI355X (profiles/r05_gemm_desc_margins.txt), worst error over limit per class: one rounding 0.987,
    + residual 0.977, GELU + residual 0.983, aux 0.986 (a bf16 rounding reaches U itself, so these sit at 1 / 1.01 by
    construction, not by a marginal kernel); two roundings 0.945; GELU 0.924; fp32 gamma 0.25 (generic kernel, K = 0,
    where gamma is 4 roundings); fp32 with activation 0.22; fp32 aux 0.03.
    """
    epi, K = case["epi"], case["K"]
    dv = want_c.device
    gc, wc = _win(got_c.to(dv).double(), case["offC"], case), _win(want_c, case["offC"], case)
    act = p["act"].abs()
    if case["dtype_c"] == gr.BF16:
        if epi == gr.EPI_GELU:
            if case["residual"]:
                ck.tight(gc, wc, tag + " C gelu+residual", rtol=ONE, mag=(p["z"] * dgelu64(p["z"])).abs() + wc.abs())
            else:
                ck.tight(gc, wc, tag + " C gelu", rtol=3 * U)
        elif case["residual"]:
            ck.tight(gc, wc, tag + " C +residual", rtol=TWO, mag=act)
        elif epi in (gr.EPI_NONE, gr.EPI_RELU, gr.EPI_DRELU):
            ck.tight(gc, wc, tag + " C one rounding", rtol=ONE)
        else:
            ck.tight(gc, wc, tag + " C two roundings", rtol=TWO)
        if epi == gr.EPI_GELU and want_x is not None:
            ck.tight(_win(got_x.to(dv).double(), case["offX"], case), _win(want_x, case["offX"], case),
                     tag + " aux one rounding", rtol=ONE)
        return
    gamma = (K + 4) * 2.0 ** -24
    if epi == gr.EPI_NONE:
        ck.tight(gc, wc, tag + " C fp32 gamma", rtol=gamma, floor=0, mag=p["mag_z"] + p["res"] + p["c_old"])
    else:
        x2 = p["x"] * p["x"] if epi >= gr.EPI_DGELU else torch.zeros_like(p["z"])
        G = p["fac"].abs() if epi >= gr.EPI_DGELU else 1.13
        mag = G * p["mag_z"] + act + p["res"] + p["c_old"] + (EPS_ACT / gamma) * p["z"].abs() * (1 + x2)
        ck.tight(gc, wc, tag + " C fp32 act", rtol=gamma, floor=0, mag=mag)
    if epi == gr.EPI_GELU and want_x is not None:
        ck.tight(_win(got_x.to(dv).double(), case["offX"], case), _win(want_x, case["offX"], case),
                 tag + " aux fp32 gamma", rtol=gamma, floor=0, mag=p["mag_z"])


@pytest.mark.parametrize("case", gr.CASES, ids=[c["name"].replace(" ", "_") for c in gr.CASES])
def test_gemm_descriptor(case):
    d = dev()
    t = _build(case, d)
    keep = {k: t[k].clone() for k in ("A", "B", "bias", "R")}
    t["C0"], t["X0"] = t["C"].clone(), t["X"].clone()
    route = _launch(case, t)
    tag = "[%s]" % gr.ROUTE_NAMES.get(route, route)
    if case["route"] is not None and not any(k in os.environ for k in SWITCHES):
        assert route == case["route"], "dispatched to %s, the table says %s" % (tag, gr.ROUTE_NAMES[case["route"]])
    got_c, got_x = t["C"].clone(), t["X"].clone()

    # ---- window: bits outside the written masks, operands
    mask, xmask = gr.window_masks(case)
    out = ~torch.from_numpy(mask).to(d)
    assert torch.equal(_bits(got_c)[out], _bits(t["C0"])[out]), "C changed outside its M x N windows"
    if xmask is not None:
        xo = ~torch.from_numpy(xmask).to(d)
        assert torch.equal(_bits(got_x)[xo], _bits(t["X0"])[xo]), "aux changed where the call may not write"
    else:
        assert torch.equal(_bits(got_x), _bits(t["X0"]))              # not passed to the call at all
    for k, v in keep.items():
        assert torch.equal(_bits(t[k]), _bits(v)), k + " changed"
    if min(case["M"], case["N"]) == 0:
        return

    # ---- values
    want_c, want_x, p = _reference(case, t)
    ck = Check()
    _check_values(ck, case, tag, got_c, got_x, want_c, want_x, p)
    del want_c, want_x, p

    # ---- a second launch from the same pre-fill: same bits unless atomics order the sums
    t["C"].copy_(t["C0"])
    t["X"].copy_(t["X0"])
    _launch(case, t)
    if not case["atomic"]:
        same = torch.equal(_bits(t["C"]), _bits(got_c)) and torch.equal(_bits(t["X"]), _bits(got_x))
        ck.rows.append("%-52s %s" % (tag + " second launch bitwise", "equal" if same else "DIFFERENT"))
        if not same:
            ck.bad.append(ck.rows[-1])
    ck.done()


def test_gemm_status_codes_leave_c_alone():
    """Every one of these returns before any launch; the descriptor is filled by hand (ops.gemm asserts on some)."""
    from focus_amd import _lib
    L = _lib.lib()
    d = dev()
    M, N, K = 64, 64, 64
    a16 = torch.ones(M * K, device=d, dtype=torch.bfloat16)
    a32 = torch.ones(M * K, device=d, dtype=torch.float32)
    b8 = torch.zeros(N * 80, device=d, dtype=torch.uint8)
    scale = torch.ones(1, device=d, dtype=torch.float32)
    ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_NULL = -1, -2, -3, -5

    def desc(A, B, C, ab, c, **kw):
        g = _lib.GemmDesc()
        g.M, g.N, g.K, g.batch0, g.batch1 = M, N, K, 1, 1
        g.A, g.rsA, g.csA = A.data_ptr(), K, 1
        g.B, g.rsB, g.csB = B.data_ptr(), 1, K
        g.C, g.rsC, g.csC = C.data_ptr(), N, 1
        g.alpha, g.dtype_ab, g.dtype_c = 1.0, ab, c
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    rows = [
        ("accumulate with bf16 C", lambda C: desc(a16, a16, C, gr.BF16, gr.BF16, accumulate=1), torch.bfloat16, ERR_DTYPE),
        ("derivative epilogue without aux", lambda C: desc(a16, a16, C, gr.BF16, gr.BF16, epilogue=gr.EPI_DGELU), torch.bfloat16, ERR_NULL),
        ("fp8 B with fp32 A", lambda C: desc(a32, b8, C, gr.F32, gr.BF16, dtype_b=gr.FP8_E4M3, b_scale=scale.data_ptr()), torch.bfloat16, ERR_DTYPE),
        ("fp8 B with csB % 16 != 0", lambda C: desc(a16, b8, C, gr.BF16, gr.BF16, dtype_b=gr.FP8_E4M3, b_scale=scale.data_ptr(), csB=72), torch.bfloat16, ERR_ALIGN),
        ("K < 0", lambda C: desc(a32, a32, C, gr.F32, gr.F32, K=-1), torch.float32, ERR_SHAPE),
        ("dtype_b differs from dtype_ab", lambda C: desc(a32, a32, C, gr.F32, gr.F32, dtype_b=gr.BF16), torch.float32, ERR_DTYPE),
    ]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for what, make, cdt, want in rows:
        C = torch.from_numpy(gr.prefill(M * N + 2 * gr.MARGIN)).to(d).to(cdt)
        C0 = C.clone()
        g = make(C)
        g.C = C.data_ptr() + gr.MARGIN * C.element_size()
        rc = L.focus_gemm(ctypes.byref(g), stream)
        torch.cuda.synchronize()
        assert rc == want, "%s: status %d, expected %d" % (what, rc, want)
        assert torch.equal(_bits(C), _bits(C0)), what + ": C was written"
