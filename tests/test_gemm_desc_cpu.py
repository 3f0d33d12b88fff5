"""The numpy reference of the focus_gemm descriptor (tests/gemm_ref.py) against hand-derived answers, and the case
table of tests/test_gpu_gemm_desc.py checked where no GPU is involved: every window inside its allocation, batch
windows disjoint, the preconditions of each expected route, coverage of routes x epilogues x output types, canary
margins.  A case that reads or writes past a buffer must fail HERE, not on a shared GPU."""
import math

import numpy as np
import pytest

import gemm_ref as gr


def _base(**kw):
    d = dict(M=2, N=2, K=3, batch=(1, 1), sA=(3, 1, 0, 0), sB=(2, 1, 0, 0), sC=(2, 1, 0, 0), offA=0, offB=0, offC=0, offR=0,
             offX=0, bias=False, residual=False, aux=False, alpha=1.0, accumulate=False, epi=gr.EPI_NONE, fp8=False,
             b_scale=1.0, tn_slab=False)
    d.update(kw)
    return d


# ----------------------------------------------------------------------------------------------------------------
# reference() against answers written out by hand
# ----------------------------------------------------------------------------------------------------------------
def test_reference_2x3x2_by_hand():
    # A = [[1,2,3],[4,5,6]]  B = [[1,0],[0,1],[2,-1]]  ->  A.B = [[7,-1],[16,-1]]
    A = np.array([1, 2, 3, 4, 5, 6], dtype=np.float32)
    B = np.array([1, 0, 0, 1, 2, -1], dtype=np.float32)
    C = np.array([10, 20, 30, 40], dtype=np.float32)
    bias = np.array([0.5, -0.5], dtype=np.float32)
    R = np.array([100, 200, 300, 400], dtype=np.float32)
    case = _base(alpha=2.0, bias=True, residual=True, accumulate=True)
    want, mask, wx, xm = gr.reference(case, dict(A=A, B=B, C=C, bias=bias, R=R))
    # 2*7+0.5+100+10, 2*-1-0.5+200+20, 2*16+0.5+300+30, 2*-1-0.5+400+40
    assert want.tolist() == [124.5, 217.5, 362.5, 437.5]
    assert mask.all() and wx is None and xm is None
    want, _, _, _ = gr.reference(_base(alpha=2.0, bias=True), dict(A=A, B=B, C=C, bias=bias))
    assert want.tolist() == [14.5, -2.5, 32.5, -2.5]          # no accumulate: C_old does not enter


def test_reference_transposed_b_view_and_offsets():
    # B stored as [N,K] rows (the nn.Linear weight): rsB = 1, csB = K, behind 2 elements of padding
    A = np.array([9, 9, 9, 1, 2, 3, 4, 5, 6], dtype=np.float32)          # offset 3
    W = np.array([7, 7, 1, 0, 2, 0, 1, -1], dtype=np.float32)            # w = [[1,0,2],[0,1,-1]] at offset 2
    C = np.full(8, -3.0, dtype=np.float32)
    case = _base(offA=3, offB=2, offC=1, sB=(1, 3, 0, 0), sC=(3, 1, 0, 0))    # row-padded C (rsC = 3 > N)
    want, mask, _, _ = gr.reference(case, dict(A=A, B=W, C=C))
    assert want.tolist() == [-3, 7, -1, -3, 16, -1, -3, -3]
    assert mask.tolist() == [False, True, True, False, True, True, False, False]


def test_reference_batched_column_sliced_c_by_loops():
    rng = np.random.RandomState(0)
    b0, b1, M, N, K = 2, 3, 4, 2, 5
    ldc = b1 * N + 2                                                 # one spare column on each side of the stripes
    sA, sB = (K, 1, b1 * M * K, M * K), (1, K, b1 * N * K, N * K)
    sC = (ldc, 1, M * ldc, N)
    A = rng.randint(-4, 5, b0 * b1 * M * K).astype(np.float32)
    B = rng.randint(-4, 5, b0 * b1 * N * K).astype(np.float32)
    offC = 3
    C = gr.prefill(offC + b0 * M * ldc + 5)
    case = _base(M=M, N=N, K=K, batch=(b0, b1), sA=sA, sB=sB, sC=sC, offC=offC + 1)
    want, mask, _, _ = gr.reference(case, dict(A=A, B=B, C=C))
    exp, emask = C.astype(np.float64).copy(), np.zeros(C.shape, bool)
    for i in range(b0):
        for j in range(b1):
            for m in range(M):
                for n in range(N):
                    acc = 0.0
                    for k in range(K):
                        acc += float(A[(i * b1 + j) * M * K + m * K + k]) * float(B[(i * b1 + j) * N * K + n * K + k])
                    pos = offC + 1 + i * M * ldc + m * ldc + j * N + n
                    exp[pos], emask[pos] = acc, True
    assert np.array_equal(want, exp) and np.array_equal(mask, emask)
    assert not mask[offC + 1 - 1] and not mask[offC + 1 + b1 * N]            # the spare columns stay unwritten
    # an independent einsum of the same form
    a4, b4 = A.reshape(b0, b1, M, K), B.reshape(b0, b1, N, K)
    e = np.einsum("ijmk,ijnk->ijmn", a4.astype(np.float64), b4.astype(np.float64))
    assert np.array_equal(gr.view(want, offC + 1, M, N, sC, b0, b1), e)


def test_reference_activation_forms_closed():
    pts = np.array([-2.0, -0.5, 0.0, 0.5, 1.0, 3.0])
    x = np.array([0.25, -1.0, 2.0, 0.0, -0.5, 1.5])
    phi = lambda t: 0.5 * (1 + math.erf(t / math.sqrt(2)))
    pdf = lambda t: math.exp(-t * t / 2) / math.sqrt(2 * math.pi)
    exp = {gr.EPI_NONE: pts, gr.EPI_GELU: [t * phi(t) for t in pts], gr.EPI_RELU: [max(t, 0.0) for t in pts],
           gr.EPI_TANH: [math.tanh(t) for t in pts],
           gr.EPI_DGELU: [t * (phi(s) + s * pdf(s)) for t, s in zip(pts, x)],
           gr.EPI_DRELU: [t if s > 0 else 0.0 for t, s in zip(pts, x)],
           gr.EPI_DTANH: [t * (1 - s * s) for t, s in zip(pts, x)]}
    for epi, e in exp.items():
        assert np.allclose(gr.activate(epi, pts, x), np.array(e, dtype=np.float64), rtol=1e-15, atol=1e-16), epi
    assert abs(gr.gelu(np.array([1.0]))[0] - 0.8413447460685429) < 1e-15          # Phi(1)
    # through reference(): 1x1x1 products v = a*b, GELU saves v in aux, DTANH reads aux and leaves it alone
    for epi in range(7):
        case = _base(M=1, N=1, K=1, sA=(1, 1, 0, 0), sB=(1, 1, 0, 0), sC=(1, 1, 0, 0), epi=epi, aux=epi in (1, 4, 5, 6),
                     residual=True)
        bufs = dict(A=np.array([3.0]), B=np.array([0.5]), C=np.array([9.0]), R=np.array([-1.0]), X=np.array([0.25]))
        want, mask, wx, xm = gr.reference(case, bufs)
        assert abs(want[0] - (gr.activate(epi, np.array([1.5]), np.array([0.25]))[0] - 1.0)) < 1e-15
        if epi == gr.EPI_GELU:
            assert wx[0] == 1.5 and xm[0]
        elif case["aux"]:
            assert wx[0] == 0.25 and not xm[0]


def test_reference_k0_is_epilogue_of_bias_plus_residual():
    case = _base(M=2, N=2, K=0, sA=(8, 1, 0, 0), sB=(1, 8, 0, 0), bias=True, residual=True, epi=gr.EPI_RELU)
    bufs = dict(A=np.zeros(4), B=np.zeros(4), C=np.array([5.0, 5, 5, 5]), bias=np.array([1.0, -2.0]), R=np.array([10.0, 20, 30, 40]))
    want, mask, _, _ = gr.reference(case, bufs)
    assert want.tolist() == [11.0, 20.0, 31.0, 40.0] and mask.all()
    want, mask, _, _ = gr.reference(_base(M=0, bias=True), bufs)
    assert want.tolist() == [5.0, 5, 5, 5] and not mask.any()


def test_torch_and_numpy_reference_agree():
    import torch
    for name in ("attn d48 att.v", "generic f32 NT epi1 Ct", "generic f32 NN epi6 acc", "K0 bf16 gelu"):
        case = gr.BY_NAME[name]
        rng = np.random.RandomState(3)
        bufs = dict(A=rng.randn(case["lenA"]).astype(np.float32), B=rng.randn(case["lenB"]).astype(np.float32),
                    C=gr.prefill(case["lenC"]), X=gr.prefill(case["lenX"])[::-1].copy(),
                    R=rng.randn(case["lenR"]).astype(np.float32), bias=rng.randn(case["lenBias"]).astype(np.float32))
        wn, mn, xn, xmn, pn = gr.reference(case, bufs, parts=True)
        tb = {k: torch.from_numpy(v) for k, v in bufs.items()}
        wt, _, xt, _, pt = gr.reference_torch(case, tb, parts=True)
        m2, xm2 = gr.window_masks(case)
        assert np.array_equal(mn, m2) and (xmn is None) == (xm2 is None) and (xmn is None or np.array_equal(xmn, xm2))
        assert np.allclose(wn, wt.numpy(), rtol=1e-13, atol=1e-13), name
        if xn is not None:
            assert np.allclose(xn, xt.numpy(), rtol=1e-13, atol=1e-13), name
        assert (pn["mag_z"] is None) == (pt["mag_z"] is None) == (case["dtype_c"] != gr.F32)    # only where a bound uses it
        for k in ("z", "mag_z", "out", "fac"):
            if pn[k] is not None:
                assert np.allclose(pn[k], pt[k].numpy(), rtol=1e-12, atol=1e-12), (name, k)


# ----------------------------------------------------------------------------------------------------------------
# the case table is safe to launch
# ----------------------------------------------------------------------------------------------------------------
def _last(off, rows, cols, s, b):
    """Independent of gemm_ref.extent: the largest element index over the corners of the window, or -1 when empty."""
    if min(rows, cols, b[0], b[1]) <= 0:
        return -1
    best = -1
    for i0 in (0, b[0] - 1):
        for i1 in (0, b[1] - 1):
            for r in (0, rows - 1):
                for c in (0, cols - 1):
                    best = max(best, off + i0 * s[2] + i1 * s[3] + r * s[0] + c * s[1])
    return best


CASE_IDS = [c["name"].replace(" ", "_") for c in gr.CASES]


@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_case_windows_stay_inside_their_buffers(case):
    M, N, K, b = case["M"], case["N"], case["K"], case["batch"]
    for s in (case["sA"], case["sB"], case["sC"]):
        assert all(v >= 0 for v in s)
    for off in ("offA", "offB", "offC", "offR", "offX"):
        assert case[off] >= 0
    assert _last(case["offA"], M, K, case["sA"], b) < case["lenA"]
    assert _last(case["offB"], K, N, case["sB"], b) < case["lenB"]
    assert _last(case["offC"], M, N, case["sC"], b) < case["lenC"]
    assert _last(case["offR"], M, N, case["sC"], b) < case["lenR"]
    if not case["tn_slab"]:                     # slab mode: the workspace is sized by the library's own query at run time
        assert _last(case["offX"], M, N, case["sC"], b) < case["lenX"]
    assert case["lenBias"] >= N
    for rows, cols, s in ((M, K, case["sA"]), (K, N, case["sB"]), (M, N, case["sC"])):
        assert gr.extent(rows, cols, s, *b) == _last(0, rows, cols, s, b) + 1
    # the MFMA kernels fetch whole 16-byte pieces of K-contiguous rows and clamp rows to M-1 / N-1: with K a multiple
    # of the piece no fetch passes the last row's end, which is what the window bound above covers


@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_case_batch_windows_of_c_are_disjoint_and_have_canaries(case):
    M, N, b = case["M"], case["N"], case["batch"]
    count = np.zeros(case["lenC"], dtype=np.int32)
    if min(M, N) > 0:
        np.add.at(count, (gr.view(np.arange(case["lenC"]), case["offC"], M, N, case["sC"], *b)).ravel(), 1)
        assert count.max() == 1, "two batch windows (or two elements of one) share an element of C"
        assert int(count.sum()) == M * N * b[0] * b[1]
    mask, xmask = gr.window_masks(case)
    assert np.array_equal(mask, count > 0)
    for mk, ln in ((mask, case["lenC"]),) + (((xmask, case["lenX"]),) if xmask is not None else ()):
        assert not mk[:gr.MARGIN].any() and not mk[ln - gr.MARGIN:].any(), "less than one tile of canary around the window"
    assert case["offC"] >= gr.MARGIN and case["offX"] >= gr.MARGIN and case["offR"] >= gr.MARGIN
    if case["col_sliced"]:
        # a row of the shared buffer: unwritten columns in front of the first stripe and behind the last one
        first = case["offC"]
        last = case["offC"] + (b[1] - 1) * case["sC"][3] + N - 1
        assert case["sC"][1] == 1 and last - first + 1 < case["sC"][0]
        assert not mask[first - 1] and not mask[last + 1]
        assert mask[first] and mask[last]
        row1 = case["sC"][0]
        assert not mask[first + row1 - 1] and not mask[last + row1 + 1] and mask[first + row1] and mask[last + row1]


def _al16(case, off, dtype):
    return (off * (2 if dtype == gr.BF16 else 4 if dtype == gr.F32 else 1)) % 16 == 0


@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_case_meets_the_preconditions_of_its_route(case):
    """Restated from the wording of include/focus_amd.h and the kernels' headers, not imported from C."""
    M, N, K, (b0, b1) = case["M"], case["N"], case["K"], case["batch"]
    sA, sB, sC = case["sA"], case["sB"], case["sC"]
    route, ab, c = case["route"], case["dtype_ab"], case["dtype_c"]
    assert route in (None, gr.GENERIC, gr.NT, gr.NT_WS, gr.TN, gr.NT_SMALL)
    assert b0 >= 1 and b1 >= 1 and b0 * b1 <= 65535
    if case["accumulate"]:
        assert c == gr.F32                                             # "1: C += result (C must be fp32)"
    if case["epi"] >= gr.EPI_DGELU:
        assert case["aux"]
    if route is None:
        assert M == 0 or N == 0
        return
    assert M > 0 and N > 0 and K >= 0
    c_aligned = _al16(case, case["offC"], c) and (not case["residual"] or _al16(case, case["offR"], c)) and \
        (not case["aux"] or case["tn_slab"] or _al16(case, case["offX"], c))
    if route in (gr.NT, gr.NT_WS, gr.NT_SMALL):
        # "The MFMA path is taken when dtype is bf16 and both A and B are contiguous along K (csA==1, rsB==1), 16-byte aligned"
        assert ab == gr.BF16 and sA[1] == 1 and sB[0] == 1
        assert K > 0 and K % 64 == 0
        assert _al16(case, case["offA"], gr.BF16) and _al16(case, case["offB"], gr.FP8_E4M3 if case["fp8"] else gr.BF16)
        assert sA[0] % 8 == 0 and sA[2] % 8 == 0 and sA[3] % 8 == 0
        q = 16 if case["fp8"] else 8                                   # e4m3 B: csB % 16 (rows of 1-byte codes)
        assert sB[1] % q == 0 and sB[2] % q == 0 and sB[3] % q == 0
        assert sA[0] >= K and sB[1] >= K
    if case["fp8"]:
        assert route == gr.NT_WS and ab == gr.BF16                     # the only consumer of e4m3 weights
    if route == gr.NT_WS:
        # bf16 out, aligned rows: 16-byte pieces of whole rows of C, aux and residual
        assert c == gr.BF16 and not case["accumulate"] and sC[1] == 1
        assert sC[0] % 8 == 0 and N % 8 == 0 and sC[2] % 8 == 0 and sC[3] % 8 == 0 and c_aligned
        assert case["tile"] in (0, 128, 160, 192)
        if case["tile"]:
            assert N >= 256 and b0 * b1 == 1 and -(-M // case["tile"]) * -(-N // 256) >= 128
    else:
        assert not case["tile"]
    if route == gr.NT_SMALL:
        # "M <= 1024 rows"; K <= 3 passes of 1536; dense C rows; one 32x32 tile per workgroup
        assert M <= 1024 and K <= 4608 and K % 32 == 0 and not case["accumulate"] and sC[1] == 1
        assert sC[0] % 4 == 0 and sC[2] % 4 == 0 and sC[3] % 4 == 0 and c_aligned
        assert -(-M // 32) * -(-N // 32) <= 4096
    if route == gr.NT:
        assert sC[1] == 1 or case["epi"] == gr.EPI_NONE
        if c == gr.F32 or sC[0] % 8 or N % 8:
            # direct epilogue: fp32 outputs, split-K atomics, layouts the LDS epilogue cannot take -- no activation
            assert case["epi"] == gr.EPI_NONE
        if case["atomic"]:
            # split-K: plain fp32-output products accumulated into C
            assert c == gr.F32 and case["accumulate"] and not case["bias"] and not case["residual"] and b0 * b1 == 1
            assert K >= 1024 and -(-M // 128) * -(-N // 128) < 256
        elif case["accumulate"]:
            assert K < 1024 or case["bias"] or case["residual"] or b0 * b1 > 1
    if route == gr.TN:
        # "A strided along the reduction: rsA == 1, csB == 1, bf16 in, fp32 out"
        assert ab == gr.BF16 and c == gr.F32 and sA[0] == 1 and sB[1] == 1 and sC[1] == 1
        assert not case["bias"] and not case["residual"] and case["epi"] == gr.EPI_NONE
        assert sA[1] % 8 == 0 and sB[0] % 8 == 0 and M % 8 == 0 and N % 8 == 0 and M >= 8 and N >= 8 and K >= 1
        assert sA[1] >= M and sB[0] >= N
        assert _al16(case, case["offA"], gr.BF16) and _al16(case, case["offB"], gr.BF16)
        if case["tn_slab"]:
            assert not case["accumulate"] and sC[0] % 4 == 0 and _al16(case, case["offC"], gr.F32)    # "C is overwritten"
        else:
            assert case["accumulate"] and case["atomic"]               # "desc->accumulate must be 1"
        if b0 * b1 > 1:
            # "batch0 == 1 ... outputs are stacked densely: rsC == N, bsC1 == M*N ... slab mode only"
            assert b0 == 1 and case["tn_slab"] and sC[0] == N and sC[3] == M * N and sA[3] % 8 == 0 and sB[3] % 8 == 0
    else:
        assert not case["tn_slab"]
    if route == gr.GENERIC:
        # no MFMA form may apply: fp32 storage, K not a multiple of 64 (or 0), an operand not K-contiguous or misaligned
        nt_layout = ab == gr.BF16 and sA[1] == 1 and sB[0] == 1 and K > 0 and K % 64 == 0 and \
            _al16(case, case["offA"], gr.BF16) and _al16(case, case["offB"], gr.BF16)
        tn_layout = ab == gr.BF16 and c == gr.F32 and sA[0] == 1 and sB[1] == 1
        assert not nt_layout and not tn_layout


def test_table_covers_every_route_epilogue_and_output_type():
    seen = {(c["route"], c["dtype_c"]) for c in gr.CASES}
    supports = {gr.GENERIC: (gr.F32, gr.BF16), gr.NT: (gr.F32, gr.BF16), gr.NT_WS: (gr.BF16,), gr.TN: (gr.F32,),
                gr.NT_SMALL: (gr.F32, gr.BF16)}
    for route, dts in supports.items():
        for dt in dts:
            assert (route, dt) in seen, (gr.ROUTE_NAMES[route], dt)
    epis = {(c["epi"], c["dtype_c"]) for c in gr.CASES}
    for e in range(7):
        assert (e, gr.BF16) in epis and (e, gr.F32) in epis, e
    # every MFMA route that takes activations meets each of them on a bf16 C
    for route in (gr.NT, gr.NT_WS):
        assert {c["epi"] for c in gr.CASES if c["route"] == route and c["dtype_c"] == gr.BF16} == set(range(7))
    assert {c["tile"] for c in gr.CASES} == {0, 128, 160, 192}
    assert any(c["fp8"] for c in gr.CASES) and any(c["K"] == 0 for c in gr.CASES)
    assert any(c["M"] == 0 for c in gr.CASES) and any(c["N"] == 0 for c in gr.CASES)
    assert any(c["tn_slab"] and c["batch"][1] > 1 for c in gr.CASES)
    assert any(c["route"] == gr.GENERIC and c["dtype_ab"] == gr.BF16 and c["sB"][1] == 1 for c in gr.CASES)   # att.v
    assert any(c["batch"][0] > 1 and c["batch"][1] > 1 for c in gr.CASES)
    assert 40 <= len(gr.CASES) <= 120


def test_prefill_is_exact_in_bf16_and_finite():
    p = gr.prefill(100000)
    assert np.isfinite(p).all() and not np.any(p.view(np.uint32) & 0xFFFF)
    assert (p != 0).mean() > 0.99 and np.abs(p).max() < 2.0
    assert (p[1:] != p[:-1]).all() and (p[256:] != p[:-256]).all() and (p[64:] != p[:-64]).all()
