"""Autograd operators over the C ABI of libfocus_amd.so.

Every function here enqueues hand-written HIP kernels on torch's current stream through ctypes;
PyTorch only owns memory and the autograd tape.  CPU tensors are rejected: the hot path has no
fallback (the CPU restatement lives in oracle/ and is test infrastructure only).
"""
import ctypes
import weakref

import torch

from . import _lib
from ._lib import BF16, F32, GemmDesc

EPI_NONE, EPI_GELU, EPI_RELU, EPI_TANH = _lib.EPI_NONE, _lib.EPI_GELU, _lib.EPI_RELU, _lib.EPI_TANH
_DEPI = {EPI_GELU: _lib.EPI_DGELU, EPI_RELU: _lib.EPI_DRELU, EPI_TANH: _lib.EPI_DTANH}


# --------------------------------------------------------------------------------------------------
# plumbing
# --------------------------------------------------------------------------------------------------
def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise RuntimeError("focus_amd: unsupported dtype %s (float32 or bfloat16)" % t.dtype)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("focus_amd: the hot path runs on the MI355X only (got a %s tensor); "
                               "there is no CPU fallback" % t.device)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


USE_TN_GEMM = True   # weight gradients straight from row-major activations (gemm_mfma_tn.hip)

# bench.py sets this to a list to collect (flops, start_event, end_event) for every MFMA-path GEMM launch
GEMM_TIMING = None


def _mfma_path(ta, sA, sB, K):
    """'nt' / 'tn' when the C dispatcher will take that MFMA kernel for this descriptor, else None."""
    if ta.dtype != torch.bfloat16:
        return None
    if sA[1] == 1 and sB[0] == 1 and K > 0 and K % 64 == 0 and sA[0] % 8 == 0 and sB[1] % 16 == 0:
        return "nt"
    if sA[1] == 1 and sB[0] == 1 and K > 0 and K % 64 == 0 and sA[0] % 8 == 0 and sB[1] % 8 == 0:
        return "nt"
    if sA[0] == 1 and sB[1] == 1 and sA[1] % 8 == 0 and sB[0] % 8 == 0:
        return "tn"
    return None


def gemm(M, N, K, A, sA, B, sB, C, sC, batch=(1, 1), bias=None, residual=None, aux=None, alpha=1.0,
         accumulate=False, epilogue=EPI_NONE, b_scale=None):
    """C = epi(alpha*A.B + bias) + residual.  A/B/C are (tensor, element_offset); s* = (rs, cs, bs0, bs1).
    b_scale: B holds OCP e4m3 codes (a uint8 tensor) with this per-tensor fp32 scale (device scalar); A is bf16."""
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.batch0, d.batch1 = batch
    (ta, oa), (tb, ob), (tc, oc) = A, B, C
    d.A, d.B, d.C = _p(ta, oa).value, _p(tb, ob).value, _p(tc, oc).value
    d.rsA, d.csA, d.bsA0, d.bsA1 = sA
    d.rsB, d.csB, d.bsB0, d.bsB1 = sB
    d.rsC, d.csC, d.bsC0, d.bsC1 = sC
    d.bias = bias.data_ptr() if bias is not None else None
    d.residual = (residual[0].data_ptr() + residual[1] * residual[0].element_size()) if residual is not None else None
    d.aux = (aux[0].data_ptr() + aux[1] * aux[0].element_size()) if aux is not None else None
    d.alpha = alpha
    d.accumulate = int(accumulate)
    d.epilogue = epilogue
    d.dtype_ab = _dt(ta)
    d.dtype_c = _dt(tc)
    if b_scale is not None:
        assert tb.dtype == torch.uint8 and ta.dtype == torch.bfloat16, "fp8 weights go with bf16 activations"
        d.dtype_b = _lib.FP8_E4M3
        d.b_scale = b_scale.data_ptr()
    else:
        assert ta.dtype == tb.dtype
    kind = _mfma_path(ta, sA, sB, K) if GEMM_TIMING is not None else None
    if kind:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.lib().focus_gemm(ctypes.byref(d), _stream()), "gemm")
        e1.record()
        if kind == "nt" and _lib.lib().focus_gemm_last_kernel() == 2:
            kind = "nt_ws8" if b_scale is not None else "nt_ws"   # the wave-specialised kernel (gemm_mfma_ws.hip)
        GEMM_TIMING.append((2.0 * M * N * K * batch[0] * batch[1], e0, e1, kind, (M, N, K, batch[0] * batch[1], epilogue)))
        return
    _lib.check(_lib.lib().focus_gemm(ctypes.byref(d), _stream()), "gemm")


def mm_nt(a, b, bias=None, residual=None, aux=None, epilogue=EPI_NONE, out_dtype=None, alpha=1.0, out=None, b_scale=None):
    """a [M,K] . b[N,K]^T -> [M,N]  (both K-contiguous: the MFMA layout).  b_scale: b holds e4m3 codes (see gemm)."""
    M, K = a.shape
    N = b.shape[0]
    c = out if out is not None else torch.empty(M, N, device=a.device, dtype=out_dtype or a.dtype)
    gemm(M, N, K, (a, 0), (a.stride(0), 1, 0, 0), (b, 0), (1, b.stride(0), 0, 0), (c, 0), (N, 1, 0, 0),
         bias=bias, residual=(residual, 0) if residual is not None else None,
         aux=(aux, 0) if aux is not None else None, alpha=alpha, epilogue=epilogue, b_scale=b_scale)
    return c


def mm_nn(a, b, aux=None, epilogue=EPI_NONE, alpha=1.0):
    """a [M,K] . b [K,N] -> [M,N] for row-major b (generic kernel unless the caller supplies b^T to mm_nt)."""
    M, K = a.shape
    N = b.shape[1]
    c = torch.empty(M, N, device=a.device, dtype=a.dtype)
    gemm(M, N, K, (a, 0), (a.stride(0), 1, 0, 0), (b, 0), (b.stride(0), 1, 0, 0), (c, 0), (N, 1, 0, 0),
         aux=(aux, 0) if aux is not None else None, epilogue=epilogue, alpha=alpha)
    return c


def transpose_pad(x, pad_to=64, dtype=None):
    """x [R,C] -> x^T zero-padded along R to a multiple of `pad_to`: [C, Rpad]."""
    R, Cc = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    out = torch.empty(Cc, Rp, device=x.device, dtype=dtype or x.dtype)
    _lib.check(_lib.lib().focus_transpose_pad(_p(x), _dt(x), x.stride(0), 0, _p(out), _dt(out), Rp, 0, R, Cc, 1,
                                              _stream()), "transpose_pad")
    return out


def mm_tn(a, b):
    """a[M,N]^T . b[M,K] -> [N,K] fp32 (weight gradients).  bf16 with N, K multiples of 8: the TN MFMA kernels read both
    operands row-major (no transposed copies); other bf16 shapes are re-laid K(=M)-contiguous by focus_transpose_pad
    for the NT kernel; fp32: strided generic kernel."""
    M, N = a.shape
    K = b.shape[1]
    if a.dtype == torch.bfloat16 and USE_TN_GEMM and N % 8 == 0 and K % 8 == 0 and N >= 8 and K >= 8:
        # both operands stay row-major: the TN MFMA kernel gathers its fragments with transposed LDS reads; the long
        # reduction is split over workgroups, partial tiles go to slabs and are summed by a second kernel
        c = torch.empty(N, K, device=a.device, dtype=torch.float32)
        nb = _lib.lib().focus_gemm_tn_workspace_bytes(N, K, M)
        ws = torch.empty(nb // 4, device=a.device, dtype=torch.float32)
        gemm(N, K, M, (a, 0), (1, a.stride(0), 0, 0), (b, 0), (b.stride(0), 1, 0, 0), (c, 0), (K, 1, 0, 0),
             aux=(ws, 0))
    elif a.dtype == torch.bfloat16:
        at, bt = transpose_pad(a), transpose_pad(b)
        Mp = at.shape[1]
        c = torch.zeros(N, K, device=a.device, dtype=torch.float32)
        gemm(N, K, Mp, (at, 0), (Mp, 1, 0, 0), (bt, 0), (1, Mp, 0, 0), (c, 0), (K, 1, 0, 0), accumulate=True)
    else:
        c = torch.empty(N, K, device=a.device, dtype=torch.float32)
        gemm(N, K, M, (a, 0), (1, a.stride(0), 0, 0), (b, 0), (b.stride(0), 1, 0, 0), (c, 0), (K, 1, 0, 0))
    return c


import os as _os


def wgrad_async(dy, x, want_bias):
    """(dw, db, join) of a Linear.  (A side-stream variant that overlapped dW with dX was measured 4-5 % SLOWER on
    the bench step -- the two persistent kernels evict each other's operand panels from L2 -- and was removed.)"""
    dw, db = linear_wgrad(dy, x, want_bias)
    return dw, db, None


def linear_wgrad(dy, x, want_bias):
    """(dw [N,K] fp32, db [N] fp32 or None) for y = x @ w^T + b from dy [M,N], x [M,K]: one pass over dy
    (focus_linear_wgrad: the bias gradient rides on the weight-gradient GEMM's matrix pipe)."""
    M, N = dy.shape
    K = x.shape[1]
    ok = (dy.dtype == torch.bfloat16 and USE_TN_GEMM and N % 8 == 0 and K % 8 == 0 and N >= 8 and K >= 8
          and dy.stride(1) == 1 and x.stride(1) == 1 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0)
    if not ok:
        return mm_tn(dy, x), (colsum(dy) if want_bias else None)
    L = _lib.lib()
    dw = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = torch.empty(N, device=dy.device, dtype=torch.float32) if want_bias else None
    nb = L.focus_linear_wgrad_workspace_bytes(N, K, M)
    ws = torch.empty(max(nb, 16) // 4, device=dy.device, dtype=torch.float32)
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.check(L.focus_linear_wgrad(_p(dy), _p(x), _p(dw), _p(db) if want_bias else None, _p(ws), nb, M, N, K,
                                    dy.stride(0), x.stride(0), _dt(dy), _stream()), "linear_wgrad")
    if GEMM_TIMING is not None:
        e1.record()
        GEMM_TIMING.append((2.0 * M * N * K, e0, e1, "tn", (N, K, M, 1, 0)))
    return dw, db


def colsum(x):
    M, N = x.shape
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().focus_colsum(_p(x), _p(out), M, N, x.stride(0), 0, _dt(x), _stream()), "colsum")
    return out


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    _lib.check(_lib.lib().focus_cast(_p(x), _dt(x), _p(out), _dt(out), x.numel(), _stream()), "cast")
    return out


# bf16 shadow copies of the fp32 master weights (and their transposes), refreshed when the parameter's
# version counter changes (optimizer steps are in-place).
_shadow_cache = {}
_shadow_gen = 0
_shadow_epoch = 0         # bumped whenever a shadow TENSOR is created or dropped (the fused optimizer caches their pointers)


def shadow_epoch():
    return _shadow_epoch


def invalidate_shadows():
    """Fused optimizers (torch._fused_adamw_) update parameters in place WITHOUT bumping Tensor._version, so the
    version counter alone cannot tell that a bf16 shadow is stale.  construct_optimizer() registers this as an
    optimizer post-step hook; call it yourself after any other out-of-band parameter update.
    The bf16 shadows that already exist (row-major and transposed) are rewritten right here by ONE multi-tensor
    launch (focus_shadow_refresh) instead of ~200 cast / transpose launches spread over the next step."""
    global _shadow_gen
    _shadow_gen += 1
    _refresh_shadows_batched()
    if _stacked:
        refresh_stacked()
    if _fp8_cache:
        refresh_fp8_shadows()


_shadow_tables = {}      # device -> (signature, items tensor, max_rows, max_cols, [(key, weakref)])


def _refresh_shadows_batched():
    import numpy as np
    by_dev = {}
    for key, (ref, stamp, out) in list(_shadow_cache.items()):
        w = ref()
        if w is None or key[1] != torch.bfloat16 or w.dtype != torch.float32 or w.dim() != 2 or not w.is_cuda:
            continue
        if w.shape[0] % 4 or w.shape[1] % 4 or not w.is_contiguous() or w.data_ptr() % 16:
            continue
        by_dev.setdefault(w.device, {}).setdefault(id(w), [w, None, None])[2 if key[2] else 1] = (key, out)
    for dev, ws in by_dev.items():
        sig = tuple((i, e[0].data_ptr(), e[1][1].data_ptr() if e[1] else 0, e[2][1].data_ptr() if e[2] else 0)
                    for i, e in sorted(ws.items()))
        tab = _shadow_tables.get(dev)
        if tab is None or tab[0] != sig:
            rec = np.zeros((len(sig), 4), dtype=np.int64)       # focus_shadow_item: 3 pointers + (rows, cols)
            mr = mc = 0
            for n, (i, sp, dp, tp) in enumerate(sig):
                w = ws[i][0]
                rec[n, 0], rec[n, 1], rec[n, 2] = sp, dp, tp
                rec[n, 3] = int(w.shape[0]) | (int(w.shape[1]) << 32)
                mr, mc = max(mr, w.shape[0]), max(mc, w.shape[1])
            tab = (sig, torch.from_numpy(rec).to(dev), mr, mc)
            _shadow_tables[dev] = tab
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().focus_shadow_refresh(_p(tab[1]), len(sig), tab[2], tab[3], _stream()), "shadow_refresh")
        for e in ws.values():
            w = e[0]
            for slot in (e[1], e[2]):
                if slot is not None:
                    key, out = slot
                    _shadow_cache[key] = (_shadow_cache[key][0], (w._version, w.data_ptr(), _shadow_gen), out)


def cached_shadow(w, dtype, transposed):
    """The existing shadow tensor of `w` (stale or not), or None: the fused optimizer step (optimizer.FusedAdamW)
    rewrites these in the same pass that updates the masters."""
    hit = _shadow_cache.get((id(w), dtype, transposed))
    if hit is not None and hit[0]() is w:
        return hit[2]
    return None


def shadows_written(entries):
    """entries: [(w, dst or None, dstT or None)] -- the bf16 shadows the optimizer step has just rewritten from the
    updated masters.  Starts a new shadow generation (every other cached copy is stale now) and stamps these as fresh."""
    global _shadow_gen
    _shadow_gen += 1
    for w, dst, dstT in entries:
        for out, tr in ((dst, False), (dstT, True)):
            if out is None:
                continue
            key = (id(w), torch.bfloat16, tr)
            hit = _shadow_cache.get(key)
            if hit is not None and hit[2] is out:
                _shadow_cache[key] = (hit[0], (w._version, w.data_ptr(), _shadow_gen), out)
    if _stacked:
        refresh_stacked()
    if _fp8_cache:
        refresh_fp8_shadows()


def drop_caches():
    """Forget every bf16 weight shadow (frees their memory when a model is dropped between workloads)."""
    global _shadow_epoch
    _shadow_epoch += 1
    _shadow_cache.clear()
    _shadow_tables.clear()
    _stacked.clear()
    _fp8_cache.clear()
    _fp8_tables.clear()


def shadow(w, dtype, transposed=False):
    w = getattr(w, "_focus_base", w)          # a wgrad_group alias stands for its parameter
    if dtype == torch.float32 and not transposed:
        return w.detach()
    key = (id(w), dtype, transposed)
    hit = _shadow_cache.get(key)
    if hit is not None and hit[0]() is w and hit[1] == (w._version, w.data_ptr(), _shadow_gen):
        return hit[2]
    wd = w.detach()
    if transposed:
        N, K = wd.shape
        out = torch.empty(K, N, device=w.device, dtype=dtype)
        _lib.check(_lib.lib().focus_transpose_pad(_p(wd), _dt(wd), K, 0, _p(out), _dt(out), N, 0, N, K, 1, _stream()),
                   "shadow^T")
    else:
        out = cast(wd, dtype)
    global _shadow_epoch
    _shadow_epoch += 1
    _shadow_cache[key] = (weakref.ref(w, lambda _r, k=key: _shadow_cache.pop(k, None)),
                          (w._version, w.data_ptr(), _shadow_gen), out)
    return out


# --------------------------------------------------------------------------------------------------
# fp8 (OCP e4m3) working copies of the Linear weights: BASELINE configs[4] "fp8 MFMA weights", SURVEY 8(d) config 5
# "fp8 weights for the Linear GEMMs, bf16 activations".  One scale per tensor (amax / 448), the SAME codes in both
# orientations: the forward reads W_q [N,K], the dX GEMM its transpose [K,N]; the fp32 masters, the weight gradients
# (activations x activations) and everything else are untouched.  `with ops.fp8_weights(True):` around a forward makes
# its Linear / MLP nodes take the fp8 B operand (their backward follows what the forward used).
# --------------------------------------------------------------------------------------------------
FP8_WEIGHTS = False
_FP8_MIN_ROWS = 1024          # fewer activation rows: the bf16 small-row kernels (the fp8 instances are the large tiles)
_fp8_cache = {}               # id(w) -> [weakref, stamp, codes [N,K] uint8, codesT [K,N] uint8, scale [1] fp32]
_fp8_tables = {}              # device -> (signature, items tensor, max_rows, max_cols, amax scratch)


class fp8_weights:
    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global FP8_WEIGHTS
        self.prev = FP8_WEIGHTS
        FP8_WEIGHTS = self.on
        return self

    def __exit__(self, *exc):
        global FP8_WEIGHTS
        FP8_WEIGHTS = self.prev
        return False


def fp8_ok(w, rows, dtype):
    w = getattr(w, "_focus_base", w)
    return (FP8_WEIGHTS and dtype == torch.bfloat16 and w.dim() == 2 and w.dtype == torch.float32 and w.is_cuda
            and rows >= _FP8_MIN_ROWS and w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0 and w.is_contiguous()
            and w.data_ptr() % 16 == 0)


def _fp8_run(dev, entries):
    import numpy as np
    sig = tuple((e[2].data_ptr(), e[3].data_ptr(), e[4].data_ptr(), w.data_ptr()) for w, e in entries)
    tab = _fp8_tables.get(dev)
    if tab is None or tab[0] != sig:
        rec = np.zeros((len(entries), 5), dtype=np.int64)          # focus_fp8_item: 4 pointers + (rows, cols)
        mr = mc = 0
        for n, (w, e) in enumerate(entries):
            rec[n, 0], rec[n, 1], rec[n, 2], rec[n, 3] = w.data_ptr(), e[2].data_ptr(), e[3].data_ptr(), e[4].data_ptr()
            rec[n, 4] = int(w.shape[0]) | (int(w.shape[1]) << 32)
            mr, mc = max(mr, w.shape[0]), max(mc, w.shape[1])
        tab = (sig, torch.from_numpy(rec).to(dev), mr, mc, torch.empty(len(entries), dtype=torch.int32, device=dev))
        if len(entries) > 1:
            _fp8_tables[dev] = tab
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().focus_fp8_refresh(_p(tab[1]), len(entries), tab[2], tab[3], _p(tab[4]), _stream()), "fp8_refresh")
    for w, e in entries:
        e[1] = (w._version, w.data_ptr(), _shadow_gen)


def refresh_fp8_shadows():
    """Requantise every cached fp8 weight copy from its fp32 master (one amax + one quantise launch per device): called
    after an optimizer step, like the bf16 shadows."""
    by_dev = {}
    for key, e in list(_fp8_cache.items()):
        w = e[0]()
        if w is None:
            _fp8_cache.pop(key, None)
            continue
        by_dev.setdefault(w.device, []).append((w, e))
    for dev, entries in by_dev.items():
        _fp8_run(dev, entries)


def shadow_fp8(w, transposed=False):
    """(e4m3 codes as a uint8 tensor -- [N,K], or [K,N] when transposed --, scale [1] fp32) of the 2-D weight w [N,K]."""
    w = getattr(w, "_focus_base", w)
    e = _fp8_cache.get(id(w))
    if e is None or e[0]() is not w:
        N, K = w.shape
        e = _fp8_cache[id(w)] = [weakref.ref(w, lambda _r, k=id(w): _fp8_cache.pop(k, None)), None,
                                 torch.empty(N, K, dtype=torch.uint8, device=w.device),
                                 torch.empty(K, N, dtype=torch.uint8, device=w.device),
                                 torch.empty(1, dtype=torch.float32, device=w.device)]
        _fp8_tables.pop(w.device, None)
    if e[1] != (w._version, w.data_ptr(), _shadow_gen):
        _fp8_run(w.device, [(w.detach(), e)])
        e[1] = (w._version, w.data_ptr(), _shadow_gen)
    return (e[3] if transposed else e[2]), e[4]


# --------------------------------------------------------------------------------------------------
# MX e4m3 activations (TRAIN.FP8_ACTIVATIONS): the forward GEMMs of the fp8-weight Linears also take their INPUT in
# e4m3, with one power-of-two (E8M0) scale per 32 consecutive elements of a row (csrc/mx_quant.hip), and run the scaled
# fp8 MFMA (csrc/gemm_mx_fp8.hip).  `with ops.fp8_activations(True):` inside ops.fp8_weights(True) turns it on.  The
# quantiser is a straight-through identity: the backward of _LinearFn / _MlpFn is the fp8-weight backward (dX on the
# e4m3 weights, dW = dY^T X with the saved bf16 X); no fp8 tensor is saved.
# --------------------------------------------------------------------------------------------------
FP8_ACTIVATIONS = False


class fp8_activations:
    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global FP8_ACTIVATIONS
        self.prev = FP8_ACTIVATIONS
        FP8_ACTIVATIONS = self.on
        return self

    def __exit__(self, *exc):
        global FP8_ACTIVATIONS
        FP8_ACTIVATIONS = self.prev
        return False


def mx_ok(w, rows, dtype):
    """The MX GEMM takes this Linear: the fp8-weight path does, and K is a whole number of 128-element K-steps."""
    return fp8_ok(w, rows, dtype) and getattr(w, "_focus_base", w).shape[1] % 128 == 0


def mx_quantize(x):
    """bf16 x [M,K] (K % 32 == 0) -> (e4m3 codes [M,K] uint8, E8M0 scales [M, K/32] uint8 in rows padded to 4 bytes)."""
    _need_gpu(x)
    if x.dtype != torch.bfloat16 or x.dim() != 2:
        raise RuntimeError("focus_amd: mx_quantize takes a 2-D bfloat16 tensor")
    if x.stride(1) != 1:
        x = x.contiguous()
    M, K = x.shape
    codes = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    scales = torch.empty(M, -(-(K // 32) // 4) * 4, dtype=torch.uint8, device=x.device)[:, :K // 32]
    _lib.check(_lib.lib().focus_mx_quant(_p(x), x.stride(0), M, K, BF16, _p(codes), codes.stride(0), _p(scales),
                                         scales.stride(0), _stream()), "mx_quant")
    return codes, scales


def mm_nt_mx(xq, xs, wq, w_scale, bias=None, residual=None, aux=None, epilogue=EPI_NONE, alpha=1.0):
    """bf16 [M,N] = epi(alpha * w_scale * (dec(xq) 2^(xs - 127)) . dec(wq)^T + bias) + residual: xq, xs from mx_quantize,
    wq [N,K] e4m3 weight codes with the per-tensor device scalar w_scale (shadow_fp8)."""
    M, K = xq.shape
    N = wq.shape[0]
    c = torch.empty(M, N, device=xq.device, dtype=torch.bfloat16)
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.batch0, d.batch1 = 1, 1
    d.A, d.rsA, d.csA = xq.data_ptr(), xq.stride(0), xq.stride(1)
    d.B, d.rsB, d.csB = wq.data_ptr(), wq.stride(1), wq.stride(0)
    d.C, d.rsC, d.csC = c.data_ptr(), N, 1
    d.bias = bias.data_ptr() if bias is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.aux = aux.data_ptr() if aux is not None else None
    d.alpha = alpha
    d.epilogue = epilogue
    d.dtype_ab = d.dtype_b = _lib.FP8_E4M3
    d.dtype_c = BF16
    d.b_scale = w_scale.data_ptr()
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.check(_lib.lib().focus_gemm_mx(ctypes.byref(d), _p(xs), xs.stride(0), _stream()), "gemm_mx")
    if GEMM_TIMING is not None:
        e1.record()
        GEMM_TIMING.append((2.0 * M * N * K, e0, e1, "nt_mx", (M, N, K, 1, epilogue)))
    return c


def _mm_fp8(x2, w, bias=None, residual=None, aux=None, epilogue=EPI_NONE, alpha=1.0):
    """Forward product of an fp8-weight Linear: MX activations when the key is on and the shape qualifies, else bf16."""
    wq, sc = shadow_fp8(w)
    if FP8_ACTIVATIONS and mx_ok(w, x2.shape[0], x2.dtype):
        xq, xs = mx_quantize(x2)
        return mm_nt_mx(xq, xs, wq, sc, bias=bias, residual=residual, aux=aux, epilogue=epilogue, alpha=alpha)
    return mm_nt(x2, wq, bias=bias, residual=residual, aux=aux, epilogue=epilogue, alpha=alpha, b_scale=sc)


def _dx_from(dy, w, dtype, aux=None, epilogue=EPI_NONE, alpha=1.0, fp8=False):
    """alpha * dy [M,N] . w[N,K] -> [M,K].  fp8: the forward multiplied by the e4m3 copy of w, so does this."""
    if fp8:
        wq, sc = shadow_fp8(w, transposed=True)
        return mm_nt(dy, wq, aux=aux, epilogue=epilogue, alpha=alpha, b_scale=sc)
    if dtype == torch.bfloat16 and w.shape[0] % 64 == 0:
        return mm_nt(dy, shadow(w, dtype, transposed=True), aux=aux, epilogue=epilogue, alpha=alpha)
    return mm_nn(dy, shadow(w, dtype), aux=aux, epilogue=epilogue, alpha=alpha)


# --------------------------------------------------------------------------------------------------
# Deferred parameter gradients.  A recurrent module (STEVE's slot update: 24 frames x 3 iterations through the same
# GRU / MLP / LayerNorm parameters) applies every weight dozens of times per step; autograd would run one tiny
# weight-gradient GEMM, one bias column-sum and one accumulation add per application (~2000 launches of 5-13 us
# per STEVE step).  Inside `with deferred_wgrads():` the Linear / MLP / LayerNorm nodes recorded by the forward
# count their applications per parameter; in the backward every application only STASHES its (dY, X), and the node
# whose backward runs LAST (the count reaches zero) runs ONE weight-gradient GEMM over the stacked applications (the
# reduction over the applications becomes part of the GEMM's reduction dimension) and RETURNS it as its parameter
# gradient -- the others return None.  The sum reaches the parameter through autograd's own AccumulateGrad, so
# DistributedDataParallel's reducer hooks fire as for any other gradient.  Same sums, different association order.
# Valid when every application recorded by the forward takes part in the backward (true for the slot loop: the slots
# chain through all of them).  If some never run (loss on a subset of frames), the count never reaches zero: a
# callback at the end of the backward pass finds such leftovers and adds them to .grad directly (single process) or
# raises (multi-rank DDP, where a gradient must not bypass the reducer).
# --------------------------------------------------------------------------------------------------
_DEFER_ON = False
_DEFER_MAX_ROWS = 8192            # applications larger than this keep the immediate path (their GEMMs are efficient)
_defer_stashes = {}               # key -> _Stash, for the forward passes recorded since the last deferred_wgrads().__enter__
_leftover_queued = False


class _Stash:
    __slots__ = ("kind", "params", "alpha", "pending", "items")

    def __init__(self, kind, params, alpha):
        self.kind, self.params, self.alpha, self.pending, self.items = kind, params, alpha, 0, []


class deferred_wgrads:
    def __enter__(self):
        global _DEFER_ON, _defer_stashes, _leftover_queued
        self.prev = _DEFER_ON
        # a fresh table: stashes of an earlier forward whose backward never ran (or raised half way) are orphaned with
        # their graph instead of swallowing this step's gradients
        _defer_stashes = {}
        _leftover_queued = False
        _DEFER_ON = _os.environ.get("FOCUS_DEFER_WGRAD", "1") != "0"
        return self

    def __exit__(self, *exc):
        global _DEFER_ON
        _DEFER_ON = self.prev
        return False


def _defer_open(kind, params, rows, needed, alpha=1.0):
    """Forward side: the stash shared by all applications of `params` (a tuple of leaf parameters / None), or None when
    this application keeps the immediate path.  needed: ctx.needs_input_grad of the weight (False under no_grad and for
    frozen parameters: nothing is counted then, and nothing is written to a frozen parameter's .grad)."""
    if not _DEFER_ON or not needed or rows > _DEFER_MAX_ROWS:
        return None
    live = [p for p in params if p is not None]
    if not live or not all(p.is_leaf and p.requires_grad for p in live):
        return None
    key = (kind, alpha) + tuple(id(p) if p is not None else 0 for p in params)
    st = _defer_stashes.get(key)
    if st is None:
        st = _defer_stashes[key] = _Stash(kind, params, alpha)
    st.pending += 1
    return st


def _defer_finish(st):
    """The gradients of a complete stash: linear -> (dw, db or None); sum -> tuple of summed vectors; ln -> (dg, db)."""
    items, st.items = st.items, []
    if st.kind == "linear":
        dy = items[0][0] if len(items) == 1 else torch.cat([i[0] for i in items], 0)
        x = items[0][1] if len(items) == 1 else torch.cat([i[1] for i in items], 0)
        dw, db = linear_wgrad(dy, x, st.params[1] is not None)
        if st.alpha != 1.0:
            dw = dw * st.alpha
        return dw, db
    if st.kind == "ln":
        both = (items[0] if len(items) == 1 else torch.cat(items, 1)).sum(1)              # [2, D]
        return both[0], both[1]
    n = len(items[0])                                                                      # "sum": tuples of vectors
    return tuple(items[0][j] if len(items) == 1 else torch.stack([i[j] for i in items], 0).sum(0) for j in range(n))


def _defer_close(st, item):
    """Backward side: stash this application's contribution; the last one returns the finished gradients (a tuple, see
    _defer_finish), the others None."""
    global _leftover_queued
    st.items.append(item)
    st.pending -= 1
    if st.pending > 0:
        if not _leftover_queued:
            _leftover_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(_deferred_leftovers)
        return None
    return _defer_finish(st)


def _acc_grad(p, g):
    g = g.reshape(p.shape)
    if p.grad is None:
        p.grad = g.to(p.dtype) if g.dtype != p.dtype else g
    else:
        p.grad.add_(g)


def _deferred_leftovers():
    """End of a backward pass: stashes that hold contributions but whose count never reached zero (some application of
    the parameter took no part in this backward)."""
    global _leftover_queued
    _leftover_queued = False
    left = [st for st in _defer_stashes.values() if st.items]
    if not left:
        return
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError("focus_amd.ops.deferred_wgrads: %d parameter(s) were applied more often in the forward than in this "
                           "backward; under DistributedDataParallel their gradient would bypass the reducer "
                           "(set FOCUS_DEFER_WGRAD=0 for this loss)" % len(left))
    with torch.no_grad():
        for st in left:
            st.pending = 0
            for p, g in zip([q for q in st.params if q is not None], [g for g in _defer_finish(st) if g is not None]):
                _acc_grad(p, g)


# --------------------------------------------------------------------------------------------------
# Grouped weight gradients.  The Linear layers of one Motionformer / ORViT block (qkv, proj_q, proj, fc1, fc2, ...) each
# give 18-72 output tiles of dW with a 12552-row reduction: alone none of them fills the 256 CUs without splitting the
# reduction into slabs that a second launch sums.  Together they are ~234 tiles = one round of the machine with no split.
# `with ops.wgrad_group(params):` around a block's forward routes the parameters through ONE autograd node (_ParamGroupFn)
# that sits upstream of every Linear / MLP node using them: those nodes stash (dY, X) instead of computing dW, and the
# group node -- which autograd runs after all of them -- forms every dW and db of the block in one launch
# (focus_linear_wgrad_group, csrc/gemm_tn_group.hip) and returns them as ITS gradients: they reach the parameters
# through AccumulateGrad like any other gradient (DistributedDataParallel's hooks fire unchanged).
# --------------------------------------------------------------------------------------------------
_GROUP_ON = _os.environ.get("FOCUS_WGRAD_GROUP", "1") != "0"
_GROUP_MIN_ROWS = 4096
_GROUP_MIN_UNITS = 128
_group_stack = []
_group_tables = {}      # (device, (N, K) of the problems of a launch) -> device unit list (focus_linear_wgrad_group_plan)


class _WgradGroup:
    def __init__(self, params):
        self.params = params
        self.index = {id(p): i for i, p in enumerate(params)}
        self.alias = {}                 # id(param) -> aliased tensor produced by the group node
        self.stash = []                 # (index of w, index of b or -1, dy2, x2)


class _ParamGroupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grp, *params):
        ctx.set_materialize_grads(False)
        ctx.grp = grp
        return tuple(p.view_as(p) for p in params)

    @staticmethod
    def backward(ctx, *gs):
        grp = ctx.grp
        out = list(gs)
        stash, grp.stash = grp.stash, []
        if stash:
            for i, g in _group_flush(grp, stash).items():
                out[i] = g if out[i] is None else out[i] + g
        return (None, *out)


def _group_flush(grp, stash):
    """All dW / db of the stashed (dY, X) pairs: one grouped launch per 8 problems when they fill the machine, the
    per-Linear path otherwise.  -> {param index: gradient}."""
    L = _lib.lib()
    res = {}
    # several applications of one weight inside the group (not the case in the blocks): stack them
    by_w = {}
    for wi, bi, dy2, x2 in stash:
        by_w.setdefault((wi, bi), []).append((dy2, x2))
    probs = []
    for (wi, bi), lst in by_w.items():
        dy2 = lst[0][0] if len(lst) == 1 else torch.cat([a for a, _ in lst], 0)
        x2 = lst[0][1] if len(lst) == 1 else torch.cat([b for _, b in lst], 0)
        probs.append((wi, bi, dy2, x2))
    probs.sort(key=lambda t: -t[2].shape[0])
    # one unit streams the WHOLE reduction of its tile: a problem whose reduction is much longer than the others' (ORViT's
    # patch_to_d[2] on the 4x more RoI-cell rows) would hold a few CUs long after the rest has finished -- it keeps the
    # per-Linear path, which splits its reduction over the machine
    med = sorted(t[2].shape[0] for t in probs)[len(probs) // 2]
    for t in [t for t in probs if t[2].shape[0] > 1.5 * med]:
        probs.remove(t)
        dw, db = linear_wgrad(t[2], t[3], t[1] >= 0)
        res[t[0]] = dw
        if t[1] >= 0:
            res[t[1]] = db
    Item = _lib.WgradItem
    arr = (Item * len(probs))()
    for n, (wi, bi, dy2, x2) in enumerate(probs):
        arr[n].M, arr[n].N, arr[n].K = dy2.shape[0], dy2.shape[1], x2.shape[1]
    units = L.focus_linear_wgrad_group_units(arr, len(probs))
    if units < _GROUP_MIN_UNITS:
        for wi, bi, dy2, x2 in probs:
            dw, db = linear_wgrad(dy2, x2, bi >= 0)
            res[wi] = dw
            if bi >= 0:
                res[bi] = db
        return res
    dev = probs[0][2].device
    nw = sum(t[2].shape[1] * t[3].shape[1] for t in probs)
    nb = sum(t[2].shape[1] for t in probs if t[1] >= 0)
    flat = torch.empty(nw + nb, device=dev, dtype=torch.float32)      # the launch stores every dW and db element
    ow, ob = 0, nw
    for n, (wi, bi, dy2, x2) in enumerate(probs):
        M, N = dy2.shape
        K = x2.shape[1]
        dw = flat[ow:ow + N * K].view(N, K)
        ow += N * K
        res[wi] = dw
        arr[n].dy, arr[n].x, arr[n].dw = dy2.data_ptr(), x2.data_ptr(), dw.data_ptr()
        arr[n].ld_dy, arr[n].ld_x = dy2.stride(0), x2.stride(0)
        arr[n].db = None
        if bi >= 0:
            db = flat[ob:ob + N]
            ob += N
            res[bi] = db
            arr[n].db = db.data_ptr()
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    # at most 8 problems per launch: more are dealt to ceil(n/8) launches of about equal size (largest first)
    nch = (len(probs) + 7) // 8
    chunks = [[] for _ in range(nch)]
    load = [0] * nch
    per = [((arr[j].N + 255) // 256) * ((arr[j].K + 127) // 128) for j in range(len(probs))]
    for j in sorted(range(len(probs)), key=lambda j: -per[j]):
        c = min((c for c in range(nch) if len(chunks[c]) < 8), key=lambda c: load[c])
        chunks[c].append(j)
        load[c] += per[j]
    for ch in chunks:
        ch.sort()                                            # keeps the longest reductions first inside a launch
        sub = (Item * len(ch))(*[arr[j] for j in ch])
        sig = (dev,) + tuple((arr[j].N, arr[j].K) for j in ch)
        table = _group_tables.get(sig)
        if table is None:                                    # the unit list depends on the (N, K) sequence only
            nu = L.focus_linear_wgrad_group_units(sub, len(ch))
            host = torch.empty(nu * 8, dtype=torch.uint8).pin_memory()
            _lib.check(L.focus_linear_wgrad_group_plan(sub, len(ch), ctypes.c_void_p(host.data_ptr()), nu * 8), "wgrad_group_plan")
            table = _group_tables[sig] = host.to(dev)        # (blocking copy, once per signature)
        _lib.check(L.focus_linear_wgrad_group(sub, len(ch), _p(table), _stream()), "linear_wgrad_group")
    if GEMM_TIMING is not None:
        e1.record()
        fl = sum(2.0 * t[2].shape[0] * t[2].shape[1] * t[3].shape[1] for t in probs)
        GEMM_TIMING.append((fl, e0, e1, "tn", (len(probs), units, probs[0][2].shape[0], 1, 0)))
    return res


class wgrad_group:
    """with ops.wgrad_group(parameters of one block): ... the block's forward ...   (see the section comment above)"""

    def __init__(self, params):
        self.params = [p for p in params if p is not None]

    def __enter__(self):
        self.grp = None
        ps = self.params
        if (_GROUP_ON and torch.is_grad_enabled() and ps and all(p.requires_grad and p.is_cuda for p in ps)):
            self.grp = _WgradGroup(ps)
            for p, a in zip(ps, _ParamGroupFn.apply(self.grp, *ps)):
                a._focus_base = p
                self.grp.alias[id(p)] = a
            _group_stack.append(self.grp)
        return self

    def __exit__(self, *exc):
        if self.grp is not None:
            _group_stack.pop()
            # the aliases are referenced by the autograd graph from here on; keeping them in the group (which the group
            # node's ctx holds) would close a reference cycle through C++ autograd nodes that the collector cannot break
            self.grp.alias = {}
            self.grp = None
        return False


def _grouped(t):
    """The active group's alias of a parameter (or the tensor itself)."""
    if t is not None and _group_stack:
        a = _group_stack[-1].alias.get(id(t))
        if a is not None:
            return a
    return t


def _group_of(w, b, rows, dtype):
    """(group, index of w, index of b) when this Linear's weight gradient is left to the active group."""
    if not _group_stack or dtype != torch.bfloat16 or rows < _GROUP_MIN_ROWS or not USE_TN_GEMM:
        return None
    grp = _group_stack[-1]
    bw = getattr(w, "_focus_base", None)
    if bw is None or id(bw) not in grp.index or w.dim() != 2 or w.shape[0] % 8 or w.shape[1] % 8:
        return None
    bi = -1
    if b is not None:
        bb = getattr(b, "_focus_base", None)
        if bb is None or id(bb) not in grp.index:
            return None
        bi = grp.index[id(bb)]
    return grp, grp.index[id(bw)], bi


# --------------------------------------------------------------------------------------------------
# Linear / MLP
# --------------------------------------------------------------------------------------------------
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, residual, alpha):
        _need_gpu(x, w)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        r2 = residual.reshape(-1, w.shape[0]).contiguous() if residual is not None else None
        ctx.fp8 = fp8_ok(w, x2.shape[0], x.dtype)
        if ctx.fp8:
            y = _mm_fp8(x2, w, bias=b, residual=r2, alpha=alpha)
        else:
            y = mm_nt(x2, shadow(w, x.dtype), bias=b, residual=r2, alpha=alpha)
        ctx.save_for_backward(x2, w)
        ctx.has_b, ctx.has_r, ctx.shp, ctx.alpha = b is not None, residual is not None, shp, alpha
        ctx.defer = _defer_open("linear", (w, b), x2.shape[0], ctx.needs_input_grad[1], alpha)
        ctx.group = None
        ctx.wbase = getattr(w, "_focus_base", w)               # shadows are keyed by the parameter, not by a group alias
        if ctx.defer is None and alpha == 1.0 and ctx.needs_input_grad[1] and x2.stride(0) % 8 == 0:
            ctx.group = _group_of(w, b, x2.shape[0], x.dtype)
        return y.reshape(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, w.shape[0])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx = dw = db = None
        join = None
        want_b = ctx.has_b and ctx.needs_input_grad[2]
        if ctx.defer is not None:
            done = _defer_close(ctx.defer, (dy2, x2))
            if done is not None:
                dw, db = done
        elif ctx.group is not None:
            grp, wi, bi = ctx.group
            grp.stash.append((wi, bi if want_b else -1, dy2, x2))      # the group node forms dW / db for the whole block
        elif ctx.needs_input_grad[1]:
            dw, db, join = wgrad_async(dy2, x2, want_b)
            if ctx.alpha != 1.0:
                dw = dw * ctx.alpha
        elif want_b:
            db = colsum(dy2)
        if ctx.needs_input_grad[0]:
            dx = _dx_from(dy2, ctx.wbase, dy2.dtype, alpha=ctx.alpha, fp8=ctx.fp8).reshape(ctx.shp)
        if join is not None:
            join()
        return dx, dw, db, (dy if ctx.has_r else None), None


def linear(x, w, b=None, residual=None, alpha=1.0):
    """nn.Linear forward (+ fused residual add): y = alpha * x.w^T + b (+ residual)."""
    return _LinearFn.apply(x, _grouped(w), _grouped(b), residual, float(alpha))


class _LinearKVFn(torch.autograd.Function):
    """Two bias-free Linears of the same input (STEVE's k / v projections of a frame, steve.py:62-63).  Forward is the
    two GEMMs; the backward forms d(input) = alpha dk.Wk + dv.Wv with the second product's epilogue adding the first
    (autograd would write both [rows, Din] products and add them in a third pass: 150 MB of traffic per frame)."""

    @staticmethod
    def forward(ctx, x, wk, wv, alpha_k):
        _need_gpu(x, wk, wv)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        k = mm_nt(x2, shadow(wk, x.dtype), alpha=alpha_k)
        v = mm_nt(x2, shadow(wv, x.dtype))
        ctx.save_for_backward(x2, wk, wv)
        ctx.shp, ctx.alpha = shp, alpha_k
        return k.reshape(*shp[:-1], wk.shape[0]), v.reshape(*shp[:-1], wv.shape[0])

    @staticmethod
    def backward(ctx, dk, dv):
        x2, wk, wv = ctx.saved_tensors
        Dk, Dv = wk.shape[0], wv.shape[0]
        dk2, dv2 = dk.reshape(-1, Dk), dv.reshape(-1, Dv)
        dt = dk2.dtype
        need_x, need_wk, need_wv = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if (Dk == Dv and dt == torch.bfloat16 and Dk % 64 == 0 and dk2.stride() == (2 * Dk, 1) == dv2.stride()
                and dv2.data_ptr() == dk2.data_ptr() + Dk * dk2.element_size()):
            # the two gradients are the halves of one [rows, 2D] matrix (ops.slot_attn_step's deferred k/v gradient):
            # d(input) = [dk|dv] . [alpha Wk; Wv] and d[Wk; Wv] = [dk|dv]^T . x, each ONE product that reads [dk|dv] once
            dkv = torch.as_strided(dk2, (dk2.shape[0], 2 * Dk), (2 * Dk, 1))
            dx = dwk = dwv = None
            if need_x:
                dx = mm_nt(dkv, _stacked_wT(wk, wv, ctx.alpha, dt)).reshape(ctx.shp)
            if need_wk or need_wv:
                dw = linear_wgrad(dkv, x2, False)[0]
                dwk = dw[:Dk] * ctx.alpha if ctx.alpha != 1.0 else dw[:Dk]
                dwv = dw[Dk:]
            return dx, dwk if need_wk else None, dwv if need_wv else None, None
        dk2 = dk2 if dk2.is_contiguous() else dk2.contiguous()
        dv2 = dv2 if dv2.is_contiguous() else dv2.contiguous()
        dwk = dwv = dx = None
        if need_wk:
            dwk = linear_wgrad(dk2, x2, False)[0]
            if ctx.alpha != 1.0:
                dwk = dwk * ctx.alpha
        if need_wv:
            dwv = linear_wgrad(dv2, x2, False)[0]
        if need_x:
            if dt == torch.bfloat16 and Dk % 64 == 0 and Dv % 64 == 0:
                dx = mm_nt(dk2, shadow(wk, dt, transposed=True), alpha=ctx.alpha)
                mm_nt(dv2, shadow(wv, dt, transposed=True), residual=dx, out=dx)   # (each element: read, add, write by one lane)
            else:
                dx = _dx_from(dk2, wk, dt, alpha=ctx.alpha) + _dx_from(dv2, wv, dt)
            dx = dx.reshape(ctx.shp)
        return dx, dwk, dwv, None


_stacked = {}       # key -> [stamp, tensor, weak refs of the weights, build(out=None or the cached tensor) -> tensor]


def _stacked_get(key, ws, extra, build):
    """A weight-derived GEMM operand built from several bf16 shadows (concatenations / stacks), cached like the shadows
    themselves: valid for (version, storage) of every weight and the shadow generation.  A stale entry of unchanged shape
    is REBUILT IN PLACE (same storage): a captured HIP graph that reads the operand keeps reading the right address, and
    refresh_stacked() -- called from the optimizer's post-step hook -- does that rebuild eagerly for every live entry."""
    stamp = tuple(x for w in ws for x in (w._version, w.data_ptr())) + (extra, _shadow_gen)
    e = _stacked.get(key)
    if e is None or e[0] != stamp:
        if e is not None and all(r() is w for r, w in zip(e[2], ws)):
            t = build(e[1])
        else:
            t = build(None)
        e = _stacked[key] = [stamp, t, [weakref.ref(w) for w in ws], build]
    return e[1]


def refresh_stacked():
    """Rebuild every cached stacked operand in place from the (already refreshed) shadows."""
    for key, e in list(_stacked.items()):
        ws = [r() for r in e[2]]
        if any(w is None for w in ws):
            _stacked.pop(key, None)
            continue
        e[1] = e[3](e[1])
        e[0] = tuple(x for w in ws for x in (w._version, w.data_ptr())) + (e[0][-2], _shadow_gen)


def _stacked_wT(wk, wv, alpha, dtype):
    """[alpha Wk; Wv]^T as an NT-GEMM B operand [Din, 2D] in `dtype`."""
    def build(out):
        parts = [shadow(wk, dtype, transposed=True) * alpha, shadow(wv, dtype, transposed=True)]
        return torch.cat(parts, dim=1, out=out) if out is not None else torch.cat(parts, dim=1).contiguous()
    return _stacked_get((id(wk), id(wv), dtype), (wk, wv), alpha, build)


def linear_kv(x, wk, wv, alpha_k=1.0):
    """(alpha_k * x.wk^T, x.wv^T): two bias-free Linears of one input with a fused d(input)."""
    return _LinearKVFn.apply(x, wk, wv, float(alpha_k))


class _MlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, act):
        _need_gpu(x, w1, w2)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M = x2.shape[0]
        H = w1.shape[0]
        z = torch.empty(M, H, device=x.device, dtype=x.dtype) if act == EPI_GELU else None
        ctx.fp8 = fp8_ok(w1, M, x.dtype) and fp8_ok(w2, M, x.dtype)
        r2 = residual.reshape(-1, w2.shape[0]).contiguous() if residual is not None else None
        if ctx.fp8:
            a = _mm_fp8(x2, w1, bias=b1, aux=z, epilogue=act)
            y = _mm_fp8(a, w2, bias=b2, residual=r2)
        else:
            a = mm_nt(x2, shadow(w1, x.dtype), bias=b1, aux=z, epilogue=act)
            y = mm_nt(a, shadow(w2, x.dtype), bias=b2, residual=r2)
        ctx.save_for_backward(x2, w1, w2, a, z)
        ctx.act, ctx.shp = act, shp
        ctx.has = (b1 is not None, b2 is not None, residual is not None)
        d1 = _defer_open("linear", (w1, b1), M, ctx.needs_input_grad[1])
        d2 = _defer_open("linear", (w2, b2), M, ctx.needs_input_grad[3]) if d1 is not None else None
        if d1 is not None and d2 is None:
            d1.pending -= 1
            d1 = None
        ctx.defer = (d1, d2) if d1 is not None else None
        ctx.group = None
        ctx.wbase = (getattr(w1, "_focus_base", w1), getattr(w2, "_focus_base", w2))
        if ctx.defer is None and ctx.needs_input_grad[1] and ctx.needs_input_grad[3] and x2.stride(0) % 8 == 0:
            g1, g2 = _group_of(w1, b1, M, x.dtype), _group_of(w2, b2, M, x.dtype)
            if g1 is not None and g2 is not None:
                ctx.group = (g1, g2)
        return y.reshape(*shp[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, a, z = ctx.saved_tensors
        dy2 = dy.reshape(-1, w2.shape[0])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        join2 = join1 = None
        dfr = ctx.defer
        grp = ctx.group
        if dfr is not None:
            dw2 = db2 = None
            done = _defer_close(dfr[1], (dy2, a))
            if done is not None:
                dw2, db2 = done
        elif grp is not None:
            dw2 = db2 = None
            grp[1][0].stash.append((grp[1][1], grp[1][2] if ctx.has[1] else -1, dy2, a))
        elif ctx.needs_input_grad[3]:
            dw2, db2, join2 = wgrad_async(dy2, a, ctx.has[1])
        else:
            dw2, db2 = None, (colsum(dy2) if ctx.has[1] else None)
        # dz = (dy . w2) * act'(.) fused in the GEMM epilogue
        dz = _dx_from(dy2, ctx.wbase[1], dy2.dtype, aux=(z if ctx.act == EPI_GELU else a), epilogue=_DEPI[ctx.act], fp8=ctx.fp8)
        if dfr is not None:
            dw1 = db1 = None
            done = _defer_close(dfr[0], (dz, x2))
            if done is not None:
                dw1, db1 = done
        elif grp is not None:
            dw1 = db1 = None
            grp[0][0].stash.append((grp[0][1], grp[0][2] if ctx.has[0] else -1, dz, x2))
        elif ctx.needs_input_grad[1]:
            dw1, db1, join1 = wgrad_async(dz, x2, ctx.has[0])
        else:
            dw1, db1 = None, (colsum(dz) if ctx.has[0] else None)
        dx = _dx_from(dz, ctx.wbase[0], dz.dtype, fp8=ctx.fp8).reshape(ctx.shp) if ctx.needs_input_grad[0] else None
        for j in (join2, join1):
            if j is not None:
                j()
        return dx, dw1, db1, dw2, db2, (dy if ctx.has[2] else None), None


def mlp(x, w1, b1, w2, b2, residual=None, act=EPI_GELU):
    """Linear -> act -> Linear (+ residual): common.py:26-34 (GELU), steve.py:46-49 / transformer.py:62-66 (ReLU)."""
    return _MlpFn.apply(x, _grouped(w1), _grouped(b1), _grouped(w2), _grouped(b2), residual, act)


class _ScaleAddFn(torch.autograd.Function):
    """out = x + scale[b] * y  (per-sample scale: stochastic depth on a residual branch), one pass each way."""

    @staticmethod
    def forward(ctx, x, y, scale, keep):
        _need_gpu(x, y, scale)
        x, y = x.contiguous(), y.contiguous()
        B = x.shape[0]
        per = x.numel() // B
        out = torch.empty_like(x)
        _lib.check(_lib.lib().focus_scale_add(_p(x), _p(y), _p(scale), keep, _p(out), B, per, _dt(x), _stream()),
                   "scale_add")
        ctx.save_for_backward(scale)
        ctx.keep = keep
        return out

    @staticmethod
    def backward(ctx, dout):
        (scale,) = ctx.saved_tensors
        dout = dout.contiguous()
        B = dout.shape[0]
        dy = torch.empty_like(dout)
        _lib.check(_lib.lib().focus_scale_add(None, _p(dout), _p(scale), ctx.keep, _p(dy), B, dout.numel() // B,
                                              _dt(dout), _stream()), "scale_add_bwd")
        return dout, dy, None, None


def residual_drop_path(x, y, drop_prob, training):
    """x + drop_path(y) (common.py:46-60): the per-sample keep mask is drawn exactly as the reference draws it."""
    if drop_prob == 0.0 or not training:
        return x + y
    keep = 1.0 - drop_prob
    # mask = floor(keep + u) and mask / keep are formed inside the kernel from the draws u
    return _ScaleAddFn.apply(x, y, torch.rand(x.shape[0], dtype=torch.float32, device=x.device), keep)


# --------------------------------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------------------------------
def _ln_forward(ctx, x, gamma, beta, eps):
    _need_gpu(x, gamma)
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    rows = x2.shape[0]
    y = torch.empty_like(x2)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().focus_layernorm_fwd(_p(x2), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, D,
                                              eps, _dt(x2), _stream()), "layernorm_fwd")
    ctx.save_for_backward(x2, gamma, mean, rstd)
    ctx.shp = x.shape
    ctx.defer = _defer_open("ln", (gamma, beta), rows, ctx.needs_input_grad[1])
    return y.reshape(x.shape)


def _ln_backward(ctx, dy, dres):
    x2, gamma, mean, rstd = ctx.saved_tensors
    D = x2.shape[1]
    rows = x2.shape[0]
    dy2 = dy.reshape(-1, D)
    if not dy2.is_contiguous():
        dy2 = dy2.contiguous()
    r2 = None
    if dres is not None:
        r2 = dres.reshape(-1, D)
        if not r2.is_contiguous():
            r2 = r2.contiguous()
    L = _lib.lib()
    nblk = L.focus_layernorm_bwd_blocks(rows)
    partial = torch.empty(2, nblk, D, device=x2.device, dtype=torch.float32)
    dx = torch.empty_like(x2)
    if ctx.defer is not None:
        # recurrent module: this application only leaves its block partials; every application's partials are summed in
        # one pass at the end of the backward (no per-application finish launch)
        _lib.check(L.focus_layernorm_bwd(_p(dy2), _p(x2), _p(gamma), _p(mean), _p(rstd), _p(r2) if r2 is not None else None,
                                         _p(dx), None, None, _p(partial), rows, D, _dt(x2), _stream()), "layernorm_bwd")
        done = _defer_close(ctx.defer, partial)
        return (dx.reshape(ctx.shp),) + (done if done is not None else (None, None))
    dg = torch.empty(D, device=x2.device, dtype=torch.float32)
    db = torch.empty(D, device=x2.device, dtype=torch.float32)
    _lib.check(L.focus_layernorm_bwd(_p(dy2), _p(x2), _p(gamma), _p(mean), _p(rstd), _p(r2) if r2 is not None else None,
                                     _p(dx), _p(dg), _p(db), _p(partial), rows, D, _dt(x2), _stream()), "layernorm_bwd")
    return dx.reshape(ctx.shp), dg, db


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        return _ln_forward(ctx, x, gamma, beta, eps)

    @staticmethod
    def backward(ctx, dy):
        return (*_ln_backward(ctx, dy, None), None)


class _LayerNormForkFn(torch.autograd.Function):
    """(x, LayerNorm(x)) for a pre-norm residual block: the gradient that comes back on the residual path is added
    to the LayerNorm's input gradient inside focus_layernorm_bwd instead of by a separate autograd accumulation."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        return x.view_as(x), _ln_forward(ctx, x, gamma, beta, eps)

    @staticmethod
    def backward(ctx, dres, dy):
        if dy is None:
            return dres, None, None, None
        return (*_ln_backward(ctx, dy, dres), None)


class _UnbindFramesFn(torch.autograd.Function):
    """x [B,T,...] -> T contiguous frames.  Slicing `x[:, t]` per frame makes autograd build, for every frame, a
    zero-filled whole-video gradient and add it to the running sum (24 x (1.2 GB fill + 3.6 GB add) per STEVE step
    at the BASELINE shape: 18.6 ms of 77); here the T frame gradients are stacked once."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape, ctx.dtype, ctx.device = x.shape, x.dtype, x.device
        return tuple(x[:, t].contiguous() for t in range(x.shape[1]))

    @staticmethod
    def backward(ctx, *grads):
        B, T = ctx.shape[0], ctx.shape[1]
        out = torch.empty(ctx.shape, dtype=ctx.dtype, device=ctx.device)
        for t, g in enumerate(grads):
            if g is None:
                out[:, t].zero_()
            else:
                out[:, t].copy_(g)
        return out


def unbind_frames(x):
    """Frames of a [B,T,...] video tensor as T contiguous tensors (see _UnbindFramesFn)."""
    return _UnbindFramesFn.apply(x)


def _guard_shared(shared, what):
    """The shared-gradient nodes (FrameGrad, SlotKVGrad) hand autograd ONE gradient from the node whose backward runs last.
    That needs every node that was counted in forward to run in this backward; a loss on a subset of the frames /
    iterations (or torch.autograd.grad on an early output) leaves some unreached, and the shared gradient would silently
    never leave.  The first node of a backward pass therefore queues a check for the end of that pass: nodes still pending
    then raise instead of dropping d(inputs)."""
    if getattr(shared, "_guarded", False):
        return
    shared._guarded = True

    def check():
        shared._guarded = False
        if shared.pending != 0:
            left = shared.pending
            shared.pending = 0
            for n in ("buf", "dk", "dv"):
                if hasattr(shared, n):
                    setattr(shared, n, None)
            if hasattr(shared, "items"):
                shared.items = []
            raise RuntimeError("%s: %d of the nodes sharing this gradient were not reached by backward (a loss on a subset "
                               "of the frames / iterations?); their shared gradient would have been dropped -- give such "
                               "uses their own %s, or none" % (what, left, type(shared).__name__))
    torch.autograd.Variable._execution_engine.queue_callback(check)


class FrameGrad:
    """Whole-video gradient buffer shared by the per-frame LayerNorm nodes of one video tensor (see layer_norm_frame)."""

    def __init__(self):
        self.buf = None
        self.pending = 0
        self.frames = 0


class _FrameLayerNormFn(torch.autograd.Function):
    """LayerNorm of frame t of a [B,T,N,D] video tensor, read in place (steve.py:60 normalises the whole video, the
    slot loop consumes one frame at a time).  Forward: no x[:, t].contiguous() copy.  Backward: every frame's node
    writes its d(x) rows straight into ONE whole-video buffer (focus_layernorm_bwd_blocks_strided); the node that runs
    last hands the buffer to autograd, the others return None -- no per-frame copy, no zero-filled whole-video
    gradients summed by autograd (all T frames must be normalised through the same FrameGrad, which the slot loop does;
    frames that never ran are zero-filled)."""

    @staticmethod
    def forward(ctx, video, t, gamma, beta, eps, shared):
        _need_gpu(video, gamma)
        assert video.dim() == 4 and video.is_contiguous()
        B, T, N, D = video.shape
        rows = B * N
        y = torch.empty(B, N, D, device=video.device, dtype=video.dtype)
        mean = torch.empty(rows, device=video.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=video.device, dtype=torch.float32)
        _lib.check(_lib.lib().focus_layernorm_fwd_blocks(_p(video, t * N * D), N, T * N * D, _p(gamma), _p(beta), _p(y),
                                                         _p(mean), _p(rstd), rows, D, eps, _dt(video), _stream()),
                   "layernorm_fwd_blocks")
        ctx.save_for_backward(video, gamma, mean, rstd)
        ctx.t, ctx.shared = t, shared
        ctx.defer = _defer_open("sum", (gamma, beta), 0, ctx.needs_input_grad[2])
        shared.pending += 1
        shared.frames |= 1 << t
        return y

    @staticmethod
    def backward(ctx, dy):
        video, gamma, mean, rstd = ctx.saved_tensors
        B, T, N, D = video.shape
        rows, t, sh = B * N, ctx.t, ctx.shared
        _guard_shared(sh, "layer_norm_frame")
        dy = dy.contiguous()
        if sh.buf is None:
            sh.buf = torch.empty_like(video)
            for tt in range(T):
                if not (sh.frames >> tt) & 1:
                    sh.buf[:, tt].zero_()
        L = _lib.lib()
        nblk = L.focus_layernorm_bwd_blocks(rows)
        partial = torch.empty(2, nblk, D, device=video.device, dtype=torch.float32)
        dg = torch.empty(D, device=video.device, dtype=torch.float32)
        db = torch.empty(D, device=video.device, dtype=torch.float32)
        _lib.check(L.focus_layernorm_bwd_blocks_strided(_p(dy), _p(video, t * N * D), N, T * N * D, _p(gamma), _p(mean),
                                                        _p(rstd), _p(sh.buf, t * N * D), _p(dg), _p(db), _p(partial), rows, D,
                                                        _dt(video), _stream()), "layernorm_bwd_blocks")
        sh.pending -= 1
        out = None
        if sh.pending == 0:
            out, sh.buf, sh.frames = sh.buf, None, 0
        if ctx.defer is not None:
            done = _defer_close(ctx.defer, (dg, db))
            dg, db = done if done is not None else (None, None)
        return out, None, dg, db, None, None


def layer_norm_frame(video, t, gamma, beta, eps, shared):
    """LayerNorm(video[:, t]) -> [B,N,D]; `shared`: one FrameGrad for all frames of `video`."""
    return _FrameLayerNormFn.apply(video, t, gamma, beta, eps, shared)


def layer_norm(x, gamma, beta, eps):
    return _LayerNormFn.apply(x, gamma, beta, eps)


def layer_norm_fork(x, gamma, beta, eps):
    """-> (x_res, LayerNorm(x)): use x_res for the block's residual add (see _LayerNormForkFn)."""
    return _LayerNormForkFn.apply(x, gamma, beta, eps)


# --------------------------------------------------------------------------------------------------
# Trajectory attention
# --------------------------------------------------------------------------------------------------
class _TrajSpaceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, F_, P, heads):
        _need_gpu(qkv)
        qkv = qkv.contiguous()
        B, N, C3 = qkv.shape
        C = C3 // 3
        d = C // heads
        S = F_ * P
        assert N == S + 1
        dev, dt = qkv.device, qkv.dtype
        xt = torch.empty(B, S, F_, C, device=dev, dtype=dt)
        xdiag = torch.empty(B, S, C, device=dev, dtype=dt)
        cls_out = torch.empty(B, 1, C, device=dev, dtype=dt)
        lse = torch.empty(B, heads, S, F_, device=dev, dtype=torch.float32)
        cls_lse = torch.empty(B, heads, device=dev, dtype=torch.float32)
        L = _lib.lib()
        nb = L.focus_traj_space_workspace_bytes(B, F_, P, heads, d, _dt(qkv), 0)
        ws = torch.empty(max(nb, 16), device=dev, dtype=torch.uint8)
        _lib.check(L.focus_traj_space_fwd(_p(qkv), _p(xt), _p(xdiag), _p(cls_out), _p(lse), _p(cls_lse), _p(ws), nb,
                                          B, F_, P, heads, d, _dt(qkv), _stream()), "traj_space_fwd")
        ctx.save_for_backward(qkv, xt, cls_out, lse, cls_lse)
        ctx.dims = (B, F_, P, heads, d)
        return xt, xdiag, cls_out

    @staticmethod
    def backward(ctx, dxt, dxdiag, dcls):
        qkv, xt, cls_out, lse, cls_lse = ctx.saved_tensors
        B, F_, P, heads, d = ctx.dims
        dxt, dxdiag, dcls = dxt.contiguous(), dxdiag.contiguous(), dcls.contiguous()
        dqkv = torch.empty_like(qkv)
        L = _lib.lib()
        nb = L.focus_traj_space_workspace_bytes(B, F_, P, heads, d, _dt(qkv), 1)
        ws = torch.empty(max(nb, 16), device=qkv.device, dtype=torch.uint8)
        _lib.check(L.focus_traj_space_bwd(_p(qkv), _p(xt), _p(cls_out), _p(lse), _p(cls_lse), _p(dxt), _p(dxdiag),
                                          _p(dcls), _p(dqkv), _p(ws), nb, B, F_, P, heads, d, _dt(qkv), _stream()),
                   "traj_space_bwd")
        return dqkv, None, None, None


def traj_space(qkv, F_, P, heads):
    """(x~ [B,S,F,C], x_diag [B,S,C], cls_out [B,1,C]) from the fused qkv projection [B,1+F*P,3C]."""
    return _TrajSpaceFn.apply(qkv, F_, P, heads)


class _TrajTimeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q2, k2, xt, heads):
        _need_gpu(q2, k2, xt)
        q2, k2, xt = q2.contiguous(), k2.contiguous(), xt.contiguous()
        B, S, F_, C = xt.shape
        d = C // heads
        out = torch.empty(B, S, C, device=xt.device, dtype=xt.dtype)
        attn2 = torch.empty(B, heads, S, F_, device=xt.device, dtype=torch.float32)
        _lib.check(_lib.lib().focus_traj_time_fwd(_p(q2), _p(k2), _p(xt), _p(out), S * C, _p(attn2), B, S, F_, heads, d,
                                                  _dt(xt), _stream()), "traj_time_fwd")
        ctx.save_for_backward(q2, k2, xt, attn2)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q2, k2, xt, attn2 = ctx.saved_tensors
        B, S, F_, C = xt.shape
        dout = dout.contiguous()
        dq2, dk2, dxt = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(xt)
        _lib.check(_lib.lib().focus_traj_time_bwd(_p(q2), _p(k2), _p(xt), _p(attn2), _p(dout), S * C, _p(dq2), _p(dk2),
                                                  _p(dxt), 0, B, S, F_, ctx.heads, C // ctx.heads, _dt(xt),
                                                  _stream()), "traj_time_bwd")
        return dq2, dk2, dxt, None


def traj_time(q2, k2, xt, heads):
    return _TrajTimeFn.apply(q2, k2, xt, heads)


class _TrajTimeBlockFn(torch.autograd.Function):
    """k2 = proj_kv(x~)[..., :C] and the temporal attention (attention.py:537-549) as ONE autograd node.  x~ feeds
    both the k2 GEMM and the attention, so autograd would sum two [B,S,F,C] gradients (a 460 MB elementwise pass per
    block); here the attention's d(x~) rides into the dX GEMM  d(x~) = dk2 . Wk + d(x~)_attn  as its residual
    epilogue.  The dead v2 half of proj_kv gets its (zero) gradient rows written once instead of through a slice
    backward."""

    @staticmethod
    def forward(ctx, q2, xt, w_kv, b_kv, cls_out, heads):
        _need_gpu(q2, xt, w_kv)
        q2, xt = q2.contiguous(), xt.contiguous()
        B, S, F_, C = xt.shape
        d = C // heads
        wk = shadow(w_kv, xt.dtype)[:C]
        bk = b_kv.detach()[:C] if b_kv is not None else None
        k2 = mm_nt(xt.view(-1, C), wk, bias=bk).view(B, S, F_, C)
        # the attention rows are written straight into tokens 1.. of the [B, 1+S, C] input of `proj`; token 0 is the
        # cls row (attention.py:551 concatenates them)
        out = torch.empty(B, S + 1, C, device=xt.device, dtype=xt.dtype)
        out[:, 0].copy_(cls_out.reshape(B, C))
        attn2 = torch.empty(B, heads, S, F_, device=xt.device, dtype=torch.float32)
        _lib.check(_lib.lib().focus_traj_time_fwd(_p(q2), _p(k2), _p(xt), _p(out, C), (S + 1) * C, _p(attn2), B, S, F_,
                                                  heads, d, _dt(xt), _stream()), "traj_time_fwd")
        ctx.save_for_backward(q2, k2, xt, attn2, w_kv)
        ctx.heads, ctx.has_b, ctx.cls_shape = heads, b_kv is not None, cls_out.shape
        return out

    @staticmethod
    def backward(ctx, dcat):
        q2, k2, xt, attn2, w_kv = ctx.saved_tensors
        B, S, F_, C = xt.shape
        dcat = dcat.contiguous()                 # [B, 1+S, C]: rows 1.. are read in place (batch stride (S+1)*C)
        dq2, dk2, dxt_a = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(xt)
        _lib.check(_lib.lib().focus_traj_time_bwd(_p(q2), _p(k2), _p(xt), _p(attn2), _p(dcat, C), (S + 1) * C, _p(dq2),
                                                  _p(dk2), _p(dxt_a), 0, B, S, F_, ctx.heads, C // ctx.heads, _dt(xt),
                                                  _stream()), "traj_time_bwd")
        dk2f, xt2 = dk2.view(-1, C), xt.view(-1, C)
        dw = db = dwk = dbk = None
        join = None
        if ctx.needs_input_grad[2]:
            dwk, dbk, join = wgrad_async(dk2f, xt2, ctx.has_b and ctx.needs_input_grad[3])
        dxt = None
        if ctx.needs_input_grad[1]:
            if xt.dtype == torch.bfloat16 and C % 64 == 0:
                wt = shadow(w_kv, xt.dtype, transposed=True)            # [C_in, 2C]: columns :C are Wk^T
                dxt = mm_nt(dk2f, wt[:, :C], residual=dxt_a.view(-1, C))
            else:
                dxt = mm_nn(dk2f, shadow(w_kv, xt.dtype)[:C]).add_(dxt_a.view(-1, C))
            dxt = dxt.view(B, S, F_, C)
        if join is not None:
            join()
        if dwk is not None:
            dw = torch.empty(2 * C, C, device=xt.device, dtype=torch.float32)
            dw[:C].copy_(dwk)
            dw[C:].zero_()                      # v2 half: no output use, exactly zero gradient
            if dbk is not None:
                db = torch.zeros(2 * C, device=xt.device, dtype=torch.float32)
                db[:C].copy_(dbk)
        dcls = dcat[:, :1].reshape(ctx.cls_shape) if ctx.needs_input_grad[4] else None
        return dq2, dxt, dw, db, dcls, None


def traj_time_block(q2, xt, w_kv, b_kv, cls_out, heads):
    """[B,1+S,C] input of `proj`: row 0 = cls_out, rows 1.. = the temporal step from q2 [B,S,C], x~ [B,S,F,C] and
    the proj_kv parameters."""
    return _TrajTimeBlockFn.apply(q2, xt, w_kv, b_kv, cls_out, heads)


class _TrajTime2BlockFn(torch.autograd.Function):
    """Temporal step of attention.py:536-549 WITHOUT k2 = proj_kv(x~)[..., :C] in HBM (csrc/traj_time2.hip): the logits
    are scale * (Wk[h]^T q2[s,h,:]) . x~[s,f,:] + const_f, u = Wk[h]^T q2 is formed per 64-channel chunk on chip.
    Forward = 3 HBM-bound launches over x~; backward = 2 launches + two batched GEMMs over the heads from
    g = d(loss)/d(u) [B,S,h,C]:  dq2[:, h] = g[:, h, :] . Wk[h]^T ,  dWk[h] = q2[:, h]^T . g[:, h, :].
    Output: the [B,1+S,C] input of `proj` (row 0 = cls_out), like _TrajTimeBlockFn."""

    @staticmethod
    def forward(ctx, q2, xt, w_kv, b_kv, cls_out, heads):
        _need_gpu(q2, xt, w_kv)
        q2, xt = q2.contiguous(), xt.contiguous()
        B, S, F_, C = xt.shape
        d = C // heads
        L = _lib.lib()
        wkT = shadow(w_kv, xt.dtype, transposed=True)                   # [C_in, 2C]: columns :C are Wk^T
        out = torch.empty(B, S + 1, C, device=xt.device, dtype=xt.dtype)
        out[:, 0].copy_(cls_out.reshape(B, C))
        attn2 = torch.empty(B, S, heads, F_, device=xt.device, dtype=torch.float32)
        nb = L.focus_traj_time2_workspace_bytes(B, S, F_, heads, d)
        ws = torch.empty(nb // 4, device=xt.device, dtype=torch.float32)
        _lib.check(L.focus_traj_time2_fwd(_p(q2), _p(xt), _p(wkT), wkT.stride(0), _p(out, C), (S + 1) * C, _p(attn2),
                                          _p(ws), nb, B, S, F_, heads, d, _dt(xt), _stream()), "traj_time2_fwd")
        ctx.save_for_backward(q2, xt, attn2, w_kv)
        ctx.heads, ctx.has_b, ctx.cls_shape = heads, b_kv is not None, cls_out.shape
        return out

    @staticmethod
    def backward(ctx, dcat):
        q2, xt, attn2, w_kv = ctx.saved_tensors
        heads = ctx.heads
        B, S, F_, C = xt.shape
        d = C // heads
        dev = xt.device
        L = _lib.lib()
        dcat = dcat.contiguous()                 # [B, 1+S, C]: rows 1.. are read in place (batch stride (S+1)*C)
        wkT = shadow(w_kv, xt.dtype, transposed=True)
        dxt = torch.empty_like(xt)
        g = torch.empty(heads, B * S, C, device=dev, dtype=xt.dtype)         # head-major: each head's GEMM operand is dense
        dl = torch.empty(B, S, F_, 16, device=dev, dtype=xt.dtype)           # [.., h padded to 16]
        _lib.check(L.focus_traj_time2_bwd(_p(q2), _p(xt), _p(wkT), wkT.stride(0), _p(attn2), _p(dcat, C), (S + 1) * C,
                                          _p(dxt), _p(g), _p(dl), B, S, F_, heads, d, _dt(xt), _stream()), "traj_time2_bwd")
        R = B * S
        dq2 = dw = db = None
        if (ctx.needs_input_grad[0] and ctx.needs_input_grad[2] and L.focus_traj_time2_gw_ok(R, heads, d, _dt(xt))
                and _os.environ.get("FOCUS_TIME2_GW", "1") != "0"):
            # both consumers of g in one pass over it (csrc/traj_time2_gw.hip): g is 12x the size of dq2
            wk = shadow(w_kv, xt.dtype)                                  # [2C, C] row-major: rows :C are Wk
            dq2 = torch.empty(B, S, C, device=dev, dtype=xt.dtype)
            dw = torch.empty(2 * C, C, device=dev, dtype=torch.float32)
            nbw = L.focus_traj_time2_gw_workspace_bytes(R, heads, d)
            wsw = torch.empty(nbw // 4, device=dev, dtype=torch.float32)
            _lib.check(L.focus_traj_time2_gw(_p(g), _p(q2), _p(wk), wk.stride(0), _p(dq2), _p(dw), _p(wsw), nbw, R, heads, d,
                                             _dt(xt), _stream()), "traj_time2_gw")
            dw[C:].zero_()                      # v2 half: no output use, exactly zero gradient
            if ctx.has_b and ctx.needs_input_grad[3]:
                db = torch.zeros(2 * C, device=dev, dtype=torch.float32)   # softmax over f is shift invariant: exactly 0
            dcls = dcat[:, :1].reshape(ctx.cls_shape) if ctx.needs_input_grad[4] else None
            return dq2, dxt, dw, db, dcls, None
        if ctx.needs_input_grad[0]:
            # dq2[r, h*d+dd] = sum_c g[h,r,c] Wk[h*d+dd, c]   (one launch, batched over the heads)
            wk = shadow(w_kv, xt.dtype)                                  # [2C, C] row-major: rows :C are Wk
            dq2 = torch.empty(B, S, C, device=dev, dtype=xt.dtype)
            gemm(R, d, C, (g, 0), (C, 1, 0, R * C), (wk, 0), (1, C, 0, d * C), (dq2, 0), (C, 1, 0, d),
                 batch=(1, heads))
        if ctx.needs_input_grad[2]:
            # dWk[h*d+dd, c] = sum_r q2[r, h*d+dd] g[h,r,c]   (batched weight-gradient product; slabs summed once)
            dw = torch.empty(2 * C, C, device=dev, dtype=torch.float32)
            nbw = L.focus_gemm_tn_batched_workspace_bytes(d, C, R, heads)
            wsw = torch.empty(max(nbw, 16) // 4, device=dev, dtype=torch.float32)
            gemm(d, C, R, (q2, 0), (1, C, 0, d), (g, 0), (C, 1, 0, R * C), (dw, 0), (C, 1, 0, d * C),
                 batch=(1, heads), aux=(wsw, 0))
            dw[C:].zero_()                      # v2 half: no output use, exactly zero gradient
            if ctx.has_b and ctx.needs_input_grad[3]:
                db = torch.zeros(2 * C, device=dev, dtype=torch.float32)   # softmax over f is shift invariant: exactly 0
        dcls = dcat[:, :1].reshape(ctx.cls_shape) if ctx.needs_input_grad[4] else None
        return dq2, dxt, dw, db, dcls, None


def traj_time2_ok(xt, heads):
    """The k2-free temporal step takes bf16, head dim 64, <= 16 heads, F in {4, 8, 16} (FOCUS_TIME2=0 disables it)."""
    if _os.environ.get("FOCUS_TIME2", "1") == "0" or xt.dtype != torch.bfloat16:
        return False
    B, S, F_, C = xt.shape
    return C % heads == 0 and C // heads == 64 and heads <= 16 and F_ in (4, 8, 16)


def traj_time2_block(q2, xt, w_kv, b_kv, cls_out, heads):
    """[B,1+S,C] input of `proj` (row 0 = cls_out) from q2 [B,S,C], x~ [B,S,F,C] and the proj_kv parameters."""
    return _TrajTime2BlockFn.apply(q2, xt, w_kv, b_kv, cls_out, heads)


# --------------------------------------------------------------------------------------------------
# Small joint attention (motion stream: attention.py:369-385; slot predictor: transformer.py:23-49)
# --------------------------------------------------------------------------------------------------
class _SmallAttnFn(torch.autograd.Function):
    """softmax(scale * q k^T [causal]) [* drop] v per head as strided batched GEMMs + a row softmax; q [B,Nq,C],
    k, v [B,Nk,C] (may be views of one buffer).  `drop` [B,h,Nq,Nk] is an inverted-dropout mask (already scaled by
    1/(1-p)) applied to the probabilities (transformer.py:45), or None."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale, causal, drop):
        _need_gpu(q, k, v)
        B, N, C = q.shape
        M = k.shape[1]
        d = C // heads
        dev, dt = q.device, q.dtype
        att = torch.empty(B, heads, N, M, device=dev, dtype=dt)
        L = _lib.lib()
        ctx.heads, ctx.scale = heads, scale

        def rows_ok(t):      # [B, n, C] whose rows are ld apart with no gap between clips (dense, or a column block)
            return t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1) and t.stride(1) >= C

        ctx.fused = (not causal and drop is None and bool(L.focus_small_attn_ok(N, M, d))
                     and rows_ok(q) and rows_ok(k) and rows_ok(v))
        if ctx.fused:       # a handful of tokens (the slot predictor): the whole attention in one launch
            out = torch.empty(B, N, C, device=dev, dtype=dt)
            _lib.check(L.focus_small_attn_fwd(_p(q), _p(k), _p(v), q.stride(1), k.stride(1), v.stride(1), _p(att), _p(out), B,
                                              heads, N, M, d, scale, _dt(q), _stream()), "small_attn_fwd")
            ctx.save_for_backward(q, k, v, att, None)
            return out
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        sa = (M, 1, heads * N * M, N * M)
        gemm(N, M, d, (q, 0), (C, 1, N * C, d), (k, 0), (1, C, M * C, d), (att, 0), sa, batch=(B, heads))
        if causal:
            assert N == M, "causal self-attention"
            _lib.check(L.focus_softmax_causal_fwd(_p(att), _p(att), B * heads * N, M, M, N, scale, _dt(att), _stream()),
                       "softmax_causal_fwd")
        else:
            _lib.check(L.focus_softmax_fwd(_p(att), _p(att), B * heads * N, M, M, scale, _dt(att), _stream()),
                       "softmax_fwd")
        attd = att if drop is None else att * drop
        out = torch.empty(B, N, C, device=dev, dtype=dt)
        gemm(N, d, M, (attd, 0), sa, (v, 0), (C, 1, M * C, d), (out, 0), (C, 1, N * C, d), batch=(B, heads))
        ctx.save_for_backward(q, k, v, att, drop)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, att, drop = ctx.saved_tensors
        heads, scale = ctx.heads, ctx.scale
        B, N, C = q.shape
        M = k.shape[1]
        d = C // heads
        dout = dout.contiguous()
        if ctx.fused:
            es = q.element_size()
            if (N == M and q.stride(1) == 3 * C == k.stride(1) == v.stride(1) and k.data_ptr() == q.data_ptr() + C * es
                    and v.data_ptr() == k.data_ptr() + C * es):
                # q | k | v are the column blocks of one projection output (ops.linear_qkv): so are their gradients
                dqkv = torch.empty(B, N, 3 * C, device=q.device, dtype=q.dtype)
                dq, dk, dv = dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:]
            else:
                dq = torch.empty(q.shape, device=q.device, dtype=q.dtype)
                dk = torch.empty(k.shape, device=q.device, dtype=q.dtype)
                dv = torch.empty(v.shape, device=q.device, dtype=q.dtype)
                if not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
                    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            _lib.check(_lib.lib().focus_small_attn_bwd(_p(q), _p(k), _p(v), q.stride(1), k.stride(1), v.stride(1), _p(att),
                                                       _p(dout), _p(dq), _p(dk), _p(dv), B, heads, N, M, d, scale, _dt(q),
                                                       _stream()), "small_attn_bwd")
            return dq, dk, dv, None, None, None, None
        sa = (M, 1, heads * N * M, N * M)
        sat = (1, M, heads * N * M, N * M)
        sq = (C, 1, N * C, d)
        sk = (C, 1, M * C, d)
        attd = att if drop is None else att * drop
        datt = torch.empty_like(att)
        # dA = dout . v^T ; dV = A^T . dout
        gemm(N, M, d, (dout, 0), sq, (v, 0), (1, C, M * C, d), (datt, 0), sa, batch=(B, heads))
        dv = torch.empty_like(v)
        gemm(M, d, N, (attd, 0), sat, (dout, 0), sq, (dv, 0), sk, batch=(B, heads))
        if drop is not None:
            datt = datt * drop
        _lib.check(_lib.lib().focus_softmax_bwd(_p(datt), _p(att), _p(datt), B * heads * N, M, M, scale, _dt(att),
                                                _stream()), "softmax_bwd")
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        gemm(N, d, M, (datt, 0), sa, (k, 0), sk, (dq, 0), sq, batch=(B, heads))
        gemm(M, d, N, (datt, 0), sat, (q, 0), sq, (dk, 0), sk, batch=(B, heads))
        return dq, dk, dv, None, None, None, None


# --------------------------------------------------------------------------------------------------
# Flash attention (STEVE decoder: causal self-attention over the image tokens, transformer.py:23-49, :131-151)
# --------------------------------------------------------------------------------------------------
def flash_ok(q, k, v, heads, causal):
    """bf16 [B, n, C] row views (dense or column blocks of one projection output) with head dim 32 / 48 / 64."""
    if not (q.is_cuda and q.dtype == torch.bfloat16 and k.dtype == q.dtype and v.dtype == q.dtype and q.dim() == 3):
        return False
    C = q.shape[2]
    if C % heads:
        return False
    for t in (q, k, v):
        if t.stride(2) != 1 or t.stride(1) % 8 or t.stride(0) % 8 or t.data_ptr() % 16:
            return False
    return bool(_lib.lib().focus_flash_attn_ok(q.shape[1], k.shape[1], C // heads, _lib.BF16, int(bool(causal))))


def drop_threshold(p):
    """The 16-bit threshold the kernels compare against: p is quantised to thr / 65536 (0.1 -> 6554)."""
    thr = int(round(float(p) * 65536.0))
    assert 0 <= thr < 65536, "dropout probability out of range"
    return thr


def _flash_args(q, k, v, out, lse, heads, scale, causal, thr, seed):
    B, Nq, C = q.shape
    a = _lib.FlashArgs()
    a.q, a.k, a.v, a.out, a.lse = _p(q), _p(k), _p(v), _p(out), _p(lse)
    a.seed = _p(seed) if seed is not None else None
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), out.stride(1)
    a.bsq, a.bsk, a.bsv, a.bso = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.B, a.heads, a.Nq, a.Nk, a.d, a.dtype, a.causal = B, heads, Nq, k.shape[1], C // heads, _lib.BF16, int(bool(causal))
    a.drop_thr, a.scale = thr, scale
    return a


class _FlashAttnFn(torch.autograd.Function):
    """out = dropout(softmax(scale q k^T [+ causal mask])) v per head, nothing of size Nq x Nk in memory
    (csrc/flash_attn.hip).  `seed`: int32 [1] device tensor naming the dropout draw (None: no dropout)."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale, causal, thr, seed):
        _need_gpu(q, k, v)
        B, Nq, C = q.shape
        out = torch.empty(B, Nq, C, device=q.device, dtype=q.dtype)
        lse = torch.empty(B, heads, Nq, device=q.device, dtype=torch.float32)
        a = _flash_args(q, k, v, out, lse, heads, scale, causal, thr, seed)
        _lib.check(_lib.lib().focus_flash_attn_fwd(ctypes.byref(a), _stream()), "flash_attn_fwd")
        ctx.save_for_backward(q, k, v, out, lse, seed)
        ctx.cfg = (heads, scale, causal, thr)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, seed = ctx.saved_tensors
        heads, scale, causal, thr = ctx.cfg
        B, Nq, C = q.shape
        Nk = k.shape[1]
        dout = dout.contiguous()
        es = q.element_size()
        if (Nq == Nk and q.stride(1) == 3 * C == k.stride(1) == v.stride(1) and k.data_ptr() == q.data_ptr() + C * es
                and v.data_ptr() == k.data_ptr() + C * es):
            # q | k | v are the column blocks of one projection output (ops.linear_qkv): so are their gradients
            dqkv = torch.empty(B, Nq, 3 * C, device=q.device, dtype=q.dtype)
            dq, dk, dv = dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:]
        else:
            dq = torch.empty(B, Nq, C, device=q.device, dtype=q.dtype)
            dk = torch.empty(B, Nk, C, device=q.device, dtype=q.dtype)
            dv = torch.empty(B, Nk, C, device=q.device, dtype=q.dtype)
        delta = torch.empty(B, heads, Nq, device=q.device, dtype=torch.float32)
        a = _flash_args(q, k, v, out, lse, heads, scale, causal, thr, seed)
        a.dout, a.delta, a.dq, a.dk, a.dv = _p(dout), _p(delta), _p(dq), _p(dk), _p(dv)
        a.lddo, a.lddq, a.lddk, a.lddv = dout.stride(1), dq.stride(1), dk.stride(1), dv.stride(1)
        a.bsdo, a.bsdq, a.bsdk, a.bsdv = dout.stride(0), dq.stride(0), dk.stride(0), dv.stride(0)
        _lib.check(_lib.lib().focus_flash_attn_bwd(ctypes.byref(a), _stream()), "flash_attn_bwd")
        return dq, dk, dv, None, None, None, None, None


def flash_attention(q, k, v, heads, scale, causal=False, p=0.0, seed=None):
    """Attention over [B, n, C] rows without materialised probabilities.  p > 0: dropout on the probabilities
    (transformer.py:44-45) drawn from `seed` (int32 [1] on the device; a fresh one from torch's generator when None)."""
    thr = drop_threshold(p) if p > 0.0 else 0
    if thr and seed is None:
        seed = torch.randint(0, 2 ** 31 - 1, (1,), device=q.device, dtype=torch.int32)
    return _FlashAttnFn.apply(q, k, v, heads, scale, causal, thr, seed if thr else None)


def small_attention(q, k, v, heads, scale, causal=False, drop=None):
    return _SmallAttnFn.apply(q, k, v, heads, scale, causal, drop)


# --------------------------------------------------------------------------------------------------
# Greedy generation (STEVE.decode, steve.py:359-381): one query row against a key/value cache, and the arg-max /
# embedding that ends a step (csrc/decode_attn.hip).  Inference only: no autograd nodes.
# --------------------------------------------------------------------------------------------------
def _no_grad_inputs(what, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError("focus_amd: %s is inference only (no backward); call it under torch.no_grad() or detach its "
                           "inputs" % what)


def decode_attention_ok(max_len, d_model, heads, dtype):
    """True when ops.decode_attention takes caches of max_len rows of d_model = heads * d channels in `dtype`."""
    if dtype not in (torch.float32, torch.bfloat16) or heads < 1 or d_model % heads:
        return False
    return bool(_lib.lib().focus_decode_attn_ok(int(max_len), d_model // heads, BF16 if dtype == torch.bfloat16 else F32))


def _rows2(t, what):
    """[B, C] or [B, 1, C] with unit channel stride -> (the [B, C] view, its row stride)."""
    if t.dim() == 3:
        assert t.shape[1] == 1, "%s: one row per sequence" % what
        t = t[:, 0]
    assert t.dim() == 2 and t.stride(1) == 1, "%s: [B, C] rows with unit channel stride" % what
    return t, t.stride(0)


class Prepared:
    """Launches whose arguments do not change from one generation step to the next -- the Linear products and LayerNorms
    of a decoder block on fixed buffers -- built once and replayed with one ctypes call each.  At a few hundred rows the
    step is bound by the host: through the autograd operators above a launch costs ~20 us of Python, here ~2 us.
    Inference only; the launches go to the stream that was current when the object was made."""

    def __init__(self):
        self.calls, self.keep = [], []
        self.stream = torch.cuda.current_stream().cuda_stream

    def linear(self, x, w, out, bias=None, residual=None, epilogue=EPI_NONE):
        """out [M, N] = epi(x [M, K] . w^T + bias) + residual; w: an [N, K] operand in x's dtype (ops.shadow)."""
        M, K = x.shape
        N = w.shape[0]
        assert w.shape[1] == K and out.shape == (M, N) and x.dtype == w.dtype == out.dtype
        assert x.stride(1) == 1 and w.stride(1) == 1 and out.is_contiguous() and out is not residual
        assert residual is None or (residual.shape == out.shape and residual.is_contiguous() and residual.dtype == out.dtype)
        d = GemmDesc()
        d.M, d.N, d.K, d.batch0, d.batch1 = M, N, K, 1, 1
        d.A, d.rsA, d.csA = x.data_ptr(), x.stride(0), 1
        d.B, d.rsB, d.csB = w.data_ptr(), 1, w.stride(0)
        d.C, d.rsC, d.csC = out.data_ptr(), N, 1
        d.bias = bias.data_ptr() if bias is not None else None
        d.residual = residual.data_ptr() if residual is not None else None
        d.alpha, d.epilogue, d.dtype_ab, d.dtype_c = 1.0, epilogue, _dt(x), _dt(out)
        self.keep.append((d, x, w, out, bias, residual))
        self.calls.append((_lib.lib().focus_gemm, (ctypes.byref(d), ctypes.c_void_p(self.stream)), "gemm"))

    def layer_norm(self, x, gamma, beta, eps, out):
        rows, D = x.shape
        assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype
        stats = torch.empty(2, rows, device=x.device, dtype=torch.float32)
        self.keep.append((x, gamma, beta, out, stats))
        self.calls.append((_lib.lib().focus_layernorm_fwd, (_p(x), _p(gamma), _p(beta), _p(out), _p(stats[0]), _p(stats[1]),
                                                            rows, D, eps, _dt(x), ctypes.c_void_p(self.stream)), "layernorm_fwd"))

    def run(self):
        for fn, args, what in self.calls:
            status = fn(*args)
            if status:
                _lib.check(status, what)


def layer_norm_into(x, gamma, beta, eps, out, stats):
    """out = LayerNorm(x) for dense [rows, D] x and out, no autograd node; stats: [2, rows] fp32 scratch (mean, rstd)."""
    _need_gpu(x, out)
    rows, D = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype
    assert stats.shape == (2, rows) and stats.dtype == torch.float32 and stats.is_contiguous()
    _lib.check(_lib.lib().focus_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(out), _p(stats[0]), _p(stats[1]), rows, D, eps,
                                              _dt(x), _stream()), "layernorm_fwd")
    return out


def stacked_weights(ws, dtype):
    """The rows of several [C, Cin] weights in `dtype` as one [sum C, Cin] operand (what ops.linear_qkv multiplies by)."""
    return _stacked_cat(tuple(ws), dtype, False)


def decode_attention(q, k_new, v_new, k_cache, v_cache, len, heads, scale, out=None):
    """softmax(scale q K^T) V per head for ONE query row per sequence over rows 0 .. len-1 of the caches [B, Lmax, C].
    q [B, C] (or [B, 1, C]); with k_new / v_new (same shape; the three may be the column blocks of one ops.linear_qkv
    output) row len-1 of the caches is written from them first; with both None the caches are only read.  -> [B, C]
    (shaped like q; `out`: a dense buffer of that shape to write instead of a new tensor)."""
    _no_grad_inputs("decode_attention", q, k_new, v_new, k_cache, v_cache)
    _need_gpu(q, k_new, v_new, k_cache, v_cache)
    assert (k_new is None) == (v_new is None), "k_new and v_new come together"
    q2, ldq = _rows2(q, "q")
    B, C = q2.shape
    ldn = 0
    if k_new is not None:
        k_new, ldn = _rows2(k_new, "k_new")
        v_new, ldv = _rows2(v_new, "v_new")
        assert ldv == ldn and k_new.shape == v_new.shape == q2.shape, "k_new and v_new: rows like q's, one stride"
    assert k_cache.shape == v_cache.shape and k_cache.dim() == 3 and k_cache.shape[0] == B and k_cache.shape[2] == C
    assert k_cache.stride() == v_cache.stride() and k_cache.stride(2) == 1
    assert k_cache.dtype == v_cache.dtype == q.dtype and (k_new is None or k_new.dtype == v_new.dtype == q.dtype)
    if out is None:
        out = torch.empty(q.shape, device=q.device, dtype=q.dtype)
    else:
        assert out.shape == q.shape and out.dtype == q.dtype and out.is_contiguous() and out.is_cuda
    _lib.check(_lib.lib().focus_decode_attn(_p(q2), ldq, _p(k_new), _p(v_new), ldn, _p(k_cache), _p(v_cache), k_cache.stride(1),
                                            k_cache.stride(0), _p(out), C, B, heads, C // heads, int(len), k_cache.shape[1],
                                            float(scale), _dt(q), _stream()), "decode_attn")
    return out


def greedy_next(logits, dictionary, pe_row, out_tok=None):
    """The end of a generation step: out_tok[b] = argmax(logits[b]) (int64, lowest index on ties; out_tok may be a column
    of the [B, gen_len] token table) and the next input row dictionary[token] + pe_row in the dtype of the logits.
    logits [B, V]; dictionary [V, D] and pe_row [D] fp32.  -> x_next [B, D]; the tokens are in out_tok."""
    _no_grad_inputs("greedy_next", logits, dictionary, pe_row)
    _need_gpu(logits, dictionary, pe_row, out_tok)
    logits, ldl = _rows2(logits, "logits")
    B, V = logits.shape
    D = dictionary.shape[1]
    assert dictionary.dtype == torch.float32 and pe_row.dtype == torch.float32 and dictionary.is_contiguous()
    assert dictionary.shape[0] == V and pe_row.shape == (D,) and pe_row.is_contiguous()
    if out_tok is None:
        out_tok = torch.empty(B, device=logits.device, dtype=torch.long)
    assert out_tok.dtype == torch.long and out_tok.shape == (B,) and (B == 1 or out_tok.stride(0) >= 1)
    x = torch.empty(B, D, device=logits.device, dtype=logits.dtype)
    _lib.check(_lib.lib().focus_greedy_next(_p(logits), ldl, _p(dictionary), _p(pe_row), _p(out_tok),
                                            out_tok.stride(0) if B > 1 else 1, _p(x), D, B, V, D, _dt(logits), _stream()),
               "greedy_next")
    return x


# --------------------------------------------------------------------------------------------------
# RoIAlign, per-RoI max, box layout
# --------------------------------------------------------------------------------------------------
class _RoiAlignFn(torch.autograd.Function):
    """RoIAlign over channels-last token maps.  `feat` is either a dense map [NI, H*W, C] (tok_T == 0) or the residual
    stream itself [B, 1 + T*H*W, C] (tok_T == T): the maps of image (b, t) are then read in place behind the cls row,
    and the backward returns a gradient of the stream's shape (cls rows zero) -- no slice copy in, no slice_backward
    + zero-fill out.  rois [K,4] fp32 xyxy pixels."""

    @staticmethod
    def forward(ctx, feat, rois, roi_img, tok_T, H, W, PH, PW, scale, sampling_ratio, aligned, relu):
        _need_gpu(feat, rois, roi_img)
        feat = feat.contiguous()
        C = feat.shape[-1]
        if tok_T:
            B = feat.shape[0]
            assert feat.shape[1] == 1 + tok_T * H * W
            NI, ipb, bstride, off = B * tok_T, tok_T, (1 + tok_T * H * W) * C, C
        else:
            NI, HW, _ = feat.shape
            assert HW == H * W
            ipb, bstride, off = NI, NI * H * W * C, 0
        K = rois.shape[0]
        out = torch.empty(K, PH * PW, C, device=feat.device, dtype=feat.dtype)
        _lib.check(_lib.lib().focus_roi_align_fwd(_p(feat, off), H * W * C, ipb, bstride, _p(rois), _p(roi_img), _p(out), NI,
                                                  C, H, W, K, PH, PW, scale, sampling_ratio, int(aligned), int(relu),
                                                  _dt(feat), _stream()), "roi_align_fwd")
        ctx.relu = bool(relu)
        ctx.save_for_backward(rois, roi_img, out if relu else None)
        ctx.args = (NI, C, H, W, K, PH, PW, scale, sampling_ratio, int(aligned), feat.dtype, ipb, bstride, off, feat.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        rois, roi_img, relu_out = ctx.saved_tensors
        NI, C, H, W, K, PH, PW, scale, sr, al, dt, ipb, bstride, off, shp = ctx.args
        dout = dout.contiguous()
        L = _lib.lib()
        dfeat = torch.empty(shp, device=dout.device, dtype=dt)
        if off:
            dfeat[:, 0].zero_()                                   # cls rows: no RoI reads them
        nb = L.focus_roi_align_bwd_workspace_bytes(NI, C, H, W, PH, PW)
        ws = torch.empty(nb // 4, device=dout.device, dtype=torch.float32) if nb else None
        _lib.check(L.focus_roi_align_bwd(_p(dout), _p(relu_out), _p(rois), _p(roi_img), _p(dfeat, off), H * W * C, ipb, bstride,
                                         _p(ws), nb, NI, C, H, W, K, PH, PW, scale, sr, al, _dt(dout), _stream()),
                   "roi_align_bwd")
        return dfeat, None, None, None, None, None, None, None, None, None, None, None


def roi_align_tokens(feat, rois, roi_img, H, W, PH, PW, spatial_scale, sampling_ratio=-1, aligned=True):
    return _RoiAlignFn.apply(feat, rois, roi_img, 0, H, W, PH, PW, float(spatial_scale), sampling_ratio, aligned, False)


def roi_align_stream(x, rois, roi_img, T, H, W, PH, PW, spatial_scale, sampling_ratio=-1, aligned=True, relu=False):
    """RoIAlign of the patch tokens of the residual stream x [B, 1+T*H*W, C], read in place (image index = b*T + t).
    Shapes whose backward needs the dense atomic path (focus_roi_align_bwd_workspace_bytes > 0) take a dense copy.
    relu: max(., 0) fused into the forward store and (as a mask from the saved output) into the backward."""
    B, _, C = x.shape
    if _lib.lib().focus_roi_align_bwd_workspace_bytes(B * T, C, H, W, PH, PW):
        out = roi_align_tokens(x[:, 1:].reshape(B * T, H * W, C), rois, roi_img, H, W, PH, PW, spatial_scale,
                               sampling_ratio, aligned)
        return torch.relu(out) if relu else out
    return _RoiAlignFn.apply(x, rois, roi_img, T, H, W, PH, PW, float(spatial_scale), sampling_ratio, aligned, relu)


def roi_stream_supports_fused(x, T, H, W, PH, PW):
    """True when roi_align_stream takes the in-place separable path for this shape (then its ReLU is fused too)."""
    B, _, C = x.shape
    return _lib.lib().focus_roi_align_bwd_workspace_bytes(B * T, C, H, W, PH, PW) == 0


class _OrvitAssembleFn(torch.autograd.Function):
    """all = cat(cls, per frame [patch tokens, object tokens]) (orvit.py:145-147) and its adjoint, one pass each."""

    @staticmethod
    def forward(ctx, x, obj, T, HW):
        _need_gpu(x, obj)
        x, obj = x.contiguous(), obj.contiguous()
        B, _, C = x.shape
        O = obj.shape[2]
        assert x.shape[1] == 1 + T * HW and obj.shape[:2] == (B, T) and obj.dtype == x.dtype
        out = torch.empty(B, 1 + T * (HW + O), C, device=x.device, dtype=x.dtype)
        _lib.check(_lib.lib().focus_orvit_assemble(_p(x), _p(obj), _p(out), B, T, HW, O, C, _dt(x), _stream()),
                   "orvit_assemble")
        ctx.args = (B, T, HW, O, C)
        return out

    @staticmethod
    def backward(ctx, dall):
        B, T, HW, O, C = ctx.args
        dall = dall.contiguous()
        dx = torch.empty(B, 1 + T * HW, C, device=dall.device, dtype=dall.dtype)
        dobj = torch.empty(B, T, O, C, device=dall.device, dtype=dall.dtype)
        _lib.check(_lib.lib().focus_orvit_assemble_bwd(_p(dall), _p(dx), _p(dobj), B, T, HW, O, C, _dt(dall), _stream()),
                   "orvit_assemble_bwd")
        return dx, dobj, None, None


def orvit_assemble(x, obj, T, HW):
    """x [B,1+T*HW,C], obj [B,T,O,C] -> [B, 1+T*(HW+O), C]."""
    return _OrvitAssembleFn.apply(x, obj, T, HW)


class _OrvitMergeFn(torch.autograd.Function):
    """x + s_b * (patch/cls rows of y + [0; mm]) (orvit.py:152-169: slice, reshape copy, motion residual, cat, drop-path,
    residual add) as one pass; the adjoint writes dy (object rows zero) and dmm, dx is dout itself."""

    @staticmethod
    def forward(ctx, x, y, mm, draws, keep, T, HW):
        _need_gpu(x, y)
        x, y = x.contiguous(), y.contiguous()
        B, _, C = x.shape
        O = (y.shape[1] - 1) // T - HW
        assert y.shape[1] == 1 + T * (HW + O) and x.shape[1] == 1 + T * HW
        scale = None
        if draws is not None:                                     # stochastic depth: s_b = floor(keep + u_b) / keep
            scale = torch.floor(keep + draws) / keep
        if mm is not None:
            mm = mm.contiguous()
        out = torch.empty_like(x)
        _lib.check(_lib.lib().focus_orvit_merge(_p(x), _p(y), _p(mm) if mm is not None else None,
                                                _p(scale) if scale is not None else None, _p(out), B, T, HW, O, C, _dt(x),
                                                _stream()), "orvit_merge")
        ctx.scale = scale
        ctx.args = (B, T, HW, O, C, mm is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, HW, O, C, has_mm = ctx.args
        dout = dout.contiguous()
        dy = torch.empty(B, 1 + T * (HW + O), C, device=dout.device, dtype=dout.dtype)
        dmm = torch.empty(B, T * HW, C, device=dout.device, dtype=dout.dtype) if has_mm else None
        sc = ctx.scale
        _lib.check(_lib.lib().focus_orvit_merge_bwd(_p(dout), _p(sc) if sc is not None else None, _p(dy),
                                                    _p(dmm) if has_mm else None, B, T, HW, O, C, _dt(dout), _stream()),
                   "orvit_merge_bwd")
        return dout, dy, dmm, None, None, None, None


def orvit_merge(x, y, mm, T, HW, drop_prob=0.0, training=False):
    """x [B,1+T*HW,C] + drop_path(cat(y[:, :1], patch rows of y + mm)); y [B,1+T*(HW+O),C], mm [B,T*HW,C] or None."""
    draws = None
    keep = 1.0 - drop_prob
    if drop_prob > 0.0 and training:
        draws = torch.rand(x.shape[0], dtype=torch.float32, device=x.device)
    return _OrvitMergeFn.apply(x, y, mm, draws, keep, T, HW)


def roi_align_indices(rois, H, W, PH, PW, spatial_scale, sampling_ratio=-1, aligned=True):
    """Integer side of RoIAlign (parity export): grid [K,2], neighbours [K,PH,PW,4] int32."""
    _need_gpu(rois)
    K = rois.shape[0]
    grid = torch.empty(K, 2, device=rois.device, dtype=torch.int32)
    nbr = torch.empty(K, PH, PW, 4, device=rois.device, dtype=torch.int32)
    _lib.check(_lib.lib().focus_roi_align_indices(_p(rois), _p(grid), _p(nbr), H, W, K, PH, PW, float(spatial_scale),
                                                  sampling_ratio, int(aligned), _stream()), "roi_align_indices")
    return grid, nbr


class _CellAmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = x.contiguous()
        K, cells, C = x.shape
        y = torch.empty(K, C, device=x.device, dtype=x.dtype)
        arg = torch.empty(K, C, device=x.device, dtype=torch.int32)
        _lib.check(_lib.lib().focus_cell_amax_fwd(_p(x), _p(y), _p(arg), K, cells, C, _dt(x), _stream()), "cell_amax")
        ctx.save_for_backward(arg)
        ctx.cells = cells
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        K, C = arg.shape
        dy = dy.contiguous()
        dx = torch.empty(K, ctx.cells, C, device=dy.device, dtype=dy.dtype)
        _lib.check(_lib.lib().focus_cell_amax_bwd(_p(dy), _p(arg), _p(dx), K, ctx.cells, C, _dt(dy), _stream()),
                   "cell_amax_bwd")
        return dx


def cell_amax(x):
    """max over the cells of each RoI: [K, cells, C] -> [K, C]."""
    return _CellAmaxFn.apply(x)


class _RoiHeadPoolFn(torch.autograd.Function):
    """max over bins of RoIAlign(mean over T) of the patch tokens of x [B, cls + T*H*W, C], read in place; the backward
    returns a gradient of x's shape (cls rows zero).  rois [K,5] fp32 on the device."""

    @staticmethod
    def forward(ctx, x, rois, T, H, W, PH, PW, scale, sampling_ratio, aligned, cls):
        _need_gpu(x, rois)
        x = x.contiguous()
        B, N, C = x.shape
        if N != cls + T * H * W:
            raise ValueError("roi_head_pool: x has %d tokens, cls + T*H*W = %d" % (N, cls + T * H * W))
        K = rois.shape[0]
        L = _lib.lib()
        pooled = torch.empty(K, C, device=x.device, dtype=x.dtype)
        arg = torch.empty(K, C, device=x.device, dtype=torch.int32)
        nb = L.focus_roi_head_workspace_bytes(B, H, W, C)
        ws = torch.empty(nb // 4, device=x.device, dtype=torch.float32)
        _lib.check(L.focus_roi_head_fwd(_p(x, cls * C), N * C, _p(rois), _p(pooled), _p(arg), _p(ws), nb, B, T, H, W, C, K, PH,
                                        PW, scale, sampling_ratio, int(aligned), _dt(x), _stream()), "roi_head_fwd")
        ctx.save_for_backward(rois, arg)
        ctx.args = (B, N, C, T, H, W, K, PH, PW, scale, sampling_ratio, int(aligned), cls, x.dtype)
        ctx.mark_non_differentiable(arg)
        return pooled, arg

    @staticmethod
    def backward(ctx, dpooled, _darg):
        rois, arg = ctx.saved_tensors
        B, N, C, T, H, W, K, PH, PW, scale, sr, al, cls, dt = ctx.args
        dpooled = dpooled.contiguous().to(dt)
        dx = torch.empty(B, N, C, device=dpooled.device, dtype=dt)
        if cls:
            dx[:, :cls].zero_()                                   # cls row: no box reads it
        _lib.check(_lib.lib().focus_roi_head_bwd(_p(dpooled), _p(arg), _p(rois), _p(dx, cls * C), N * C, B, T, H, W, C, K, PH,
                                                 PW, scale, sr, al, _dt(dx), _stream()), "roi_head_bwd")
        return dx, None, None, None, None, None, None, None, None, None, None


def roi_head_boxes(rois, B, device):
    """rois [K,5] (batch index, x1, y1, x2, y2) as the fp32 device tensor the kernels read.  While the boxes are still a host
    tensor (how a loader hands them over) their batch indices are checked here, without a sync: an index that is not an
    integer in [0, B) is refused.  Boxes already on the device are taken as they are (the kernels skip such a box)."""
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError("roi_head_pool: boxes must be [K,5] (batch index, x1, y1, x2, y2), got %s" % (tuple(rois.shape),))
    if rois.device.type == "cpu":
        idx = rois[:, 0]
        if rois.shape[0] and not bool(((idx >= 0) & (idx < B) & (idx == idx.floor())).all()):
            raise ValueError("roi_head_pool: box batch index outside [0, %d) (%s: %s)" % (
                B, _lib.lib().focus_strerror(-1).decode(), idx.tolist()))
        rois = rois.to(device=device, dtype=torch.float32, non_blocking=True)
    return rois.float().contiguous()


def roi_head_pool(x, rois, T, H, W, PH, PW, spatial_scale, sampling_ratio=0, aligned=True, cls=1, return_arg=False):
    """ResNetRoIHead's pooling on the token stream: x [B, cls + T*H*W, C], rois [K,5] (batch index, x1, y1, x2, y2 in input
    pixels) -> [K, C] = MaxPool2d(PH,PW)(ROIAlign(AvgPool3d([T,1,1])(x))) without the transpose and the [K,PH*PW,C]
    intermediate (csrc/roi_head.hip).  spatial_scale multiplies the box coordinates (1 / SPATIAL_SCALE_FACTOR)."""
    rois = roi_head_boxes(rois, x.shape[0], x.device)
    pooled, arg = _RoiHeadPoolFn.apply(x, rois, int(T), int(H), int(W), int(PH), int(PW), float(spatial_scale),
                                       int(sampling_ratio), bool(aligned), int(cls))
    return (pooled, arg) if return_arg else pooled


class _BoxLayoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vecs, boxes, H, W):
        _need_gpu(vecs, boxes)
        vecs, boxes = vecs.contiguous(), boxes.contiguous().float()
        NF, O, C = vecs.shape
        out = torch.empty(NF, H * W, C, device=vecs.device, dtype=vecs.dtype)
        _lib.check(_lib.lib().focus_box_layout_fwd(_p(vecs), _p(boxes), _p(out), NF, O, C, H, W, _dt(vecs), _stream()),
                   "box_layout_fwd")
        ctx.save_for_backward(boxes)
        ctx.args = (NF, O, C, H, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        (boxes,) = ctx.saved_tensors
        NF, O, C, H, W = ctx.args
        dout = dout.contiguous()
        dv = torch.empty(NF, O, C, device=dout.device, dtype=dout.dtype)
        _lib.check(_lib.lib().focus_box_layout_bwd(_p(dout), _p(boxes), _p(dv), NF, O, C, H, W, _dt(dout), _stream()),
                   "box_layout_bwd")
        return dv, None, None, None


def box_layout(vecs, boxes, H, W):
    """vecs [NF,O,C], boxes [NF,O,4] cxcywh -> [NF, H*W, C]."""
    return _BoxLayoutFn.apply(vecs, boxes, H, W)


# --------------------------------------------------------------------------------------------------
# Motionformer embedding / loss
# --------------------------------------------------------------------------------------------------
def im2col_patches(x, kt, kh, kw, dtype):
    _need_gpu(x)
    x = x.contiguous().float()
    B, Cin, T, H, W = x.shape
    rows = B * (T // kt) * (H // kh) * (W // kw)
    cols = torch.empty(rows, Cin * kt * kh * kw, device=x.device, dtype=dtype)
    _lib.check(_lib.lib().focus_im2col_patches(_p(x), _p(cols), B, Cin, T, H, W, kt, kh, kw, _dt(cols), _stream()),
               "im2col")
    return cols


class _EmbedAssembleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, patch, cls, pos, temp):
        _need_gpu(patch, cls, pos, temp)
        B, S, C = patch.shape
        T = temp.shape[0]
        P = S // T
        patch = patch.contiguous()
        tok = torch.empty(B, 1 + S, C, device=patch.device, dtype=patch.dtype)
        _lib.check(_lib.lib().focus_embed_assemble(_p(patch), _p(cls), _p(pos), _p(temp), _p(tok), B, T, P, C,
                                                   _dt(patch), _stream()), "embed_assemble")
        ctx.dims = (B, T, P, C)
        return tok

    @staticmethod
    def backward(ctx, dtok):
        # adjoint = slices and small reductions over the batch: parameter-gradient plumbing
        B, T, P, C = ctx.dims
        g = dtok.float()
        gp = g[:, 1:].reshape(B, T, P, C)
        dcls = g[:, 0].sum(0)
        dpos = torch.cat([dcls[None], gp.sum((0, 1))], 0)
        dtemp = gp.sum((0, 2))
        return dtok[:, 1:], dcls, dpos, dtemp


def embed_assemble(patch, cls, pos, temp):
    """cls [C], pos [1+P,C], temp [T,C] fp32 parameters."""
    return _EmbedAssembleFn.apply(patch, cls.contiguous(), pos.contiguous(), temp.contiguous())


def rows_ok(t):
    """[R, V] rows the one-workgroup-per-row passes of gumbel.hip take: dense, fp32 or bf16, V % 8 == 0, V <= 8192."""
    return (t.is_cuda and t.dim() == 2 and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16)
            and t.data_ptr() % 16 == 0 and bool(_lib.lib().focus_rows_ok(t.shape[0], t.shape[1], _dt(t))))


class _XentLsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, smoothing):
        _need_gpu(logits, target)
        ctx.rows = rows_ok(logits)
        R, Ncls = logits.shape
        loss_rows = torch.empty(R, device=logits.device, dtype=torch.float32)
        if ctx.rows:
            # fp32 or bf16 logits as they are; the backward rebuilds softmax from the row log-sum-exp instead of keeping an
            # fp32 [R, V] gradient alive (STEVE's decoder head: 196608 x 4096 per 8 clips)
            target = target.contiguous()
            lse = torch.empty(R, device=logits.device, dtype=torch.float32)
            _lib.check(_lib.lib().focus_xent_rows_fwd(_p(logits), _p(target), _p(loss_rows), _p(lse), R, Ncls, smoothing,
                                                      _dt(logits), _stream()), "xent_rows_fwd")
            ctx.save_for_backward(logits, target, lse)
            ctx.smoothing = smoothing
            return loss_rows.mean()
        logits = logits.float().contiguous()
        dlog = torch.empty_like(logits)
        _lib.check(_lib.lib().focus_xent_ls(_p(logits), _p(target.contiguous()), _p(loss_rows), _p(dlog), R, Ncls,
                                            smoothing, _stream()), "xent_ls")
        ctx.save_for_backward(dlog)
        return loss_rows.mean()

    @staticmethod
    def backward(ctx, g):
        if ctx.rows:
            logits, target, lse = ctx.saved_tensors
            dlog = torch.empty_like(logits)
            g = g.to(torch.float32).contiguous()
            _lib.check(_lib.lib().focus_xent_rows_bwd(_p(logits), _p(target), _p(lse), _p(g), _p(dlog), logits.shape[0],
                                                      logits.shape[1], ctx.smoothing, _dt(logits), _stream()), "xent_rows_bwd")
            return dlog, None, None
        (dlog,) = ctx.saved_tensors
        return dlog * g, None, None


def label_smoothing_ce(logits, target, smoothing=0.1):
    return _XentLsFn.apply(logits, target, smoothing)


# --------------------------------------------------------------------------------------------------
# residual + dropout(branch) (the decoder blocks of STEVE: transformer.py:45-47, :147-163)
# --------------------------------------------------------------------------------------------------
class _DropoutAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, residual, thr, seed):
        out = torch.empty_like(y)
        _lib.check(_lib.lib().focus_dropout_add(_p(y), _p(residual) if residual is not None else None, _p(seed), thr, _p(out),
                                                y.numel(), _dt(y), _stream()), "dropout_add")
        ctx.save_for_backward(seed)
        ctx.thr, ctx.has_res = thr, residual is not None
        return out

    @staticmethod
    def backward(ctx, g):
        (seed,) = ctx.saved_tensors
        g = g.contiguous()
        dy = torch.empty_like(g)
        _lib.check(_lib.lib().focus_dropout_add(_p(g), None, _p(seed), ctx.thr, _p(dy), g.numel(), _dt(g), _stream()),
                   "dropout_add_bwd")
        return dy, (g if ctx.has_res else None), None, None


def dropout_add(y, residual, p, training, seed=None):
    """residual + F.dropout(y, p, training) (residual may be None).  On the GPU, for dense fp32 / bf16 tensors, one pass whose
    mask is a hash of (seed, element index) -- rebuilt by the backward, never stored; `seed`: int32 [2] on the device
    (default: drawn from torch's generator).  p is quantised to drop_threshold(p) / 65536."""
    if not training or p <= 0.0:
        return y if residual is None else residual + y
    _need_gpu(y, residual)
    thr = drop_threshold(p)
    # (shapes the kernel does not take -- odd element counts, strided views -- keep ATen's dropout, on the GPU)
    ok = (y.is_contiguous() and y.dtype in (torch.float32, torch.bfloat16) and y.numel() % 8 == 0
          and y.numel() > 0 and y.data_ptr() % 16 == 0 and thr > 0
          and (residual is None or (residual.shape == y.shape and residual.dtype == y.dtype and residual.is_contiguous()
                                    and residual.data_ptr() % 16 == 0)))
    if not ok:
        out = torch.nn.functional.dropout(y, p, True)
        return out if residual is None else residual + out
    if seed is None:
        seed = torch.randint(-2 ** 31, 2 ** 31 - 1, (2,), device=y.device, dtype=torch.int32)
    return _DropoutAddFn.apply(y, residual, thr, seed)


# --------------------------------------------------------------------------------------------------
# Gumbel-softmax over the dVAE vocabulary (steve.py:262-271, STEVE/utils.py:47-61)
# --------------------------------------------------------------------------------------------------
class _GumbelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tau, hard, e_soft, e_hard, want_target, seed, out_dtype):
        _need_gpu(x)
        R, V = x.shape
        dev = x.device
        gen = e_soft is None
        if gen:
            # the draws are made in the kernel from this seed (and made again by the backward); the seed itself comes from
            # torch's generator, on the device, so that a captured step draws fresh noise on every replay
            if seed is None:
                seed = torch.randint(-2 ** 31, 2 ** 31 - 1, (4,), device=dev, dtype=torch.int32)
            assert seed.dtype == torch.int32 and seed.numel() == 4 and seed.is_cuda and seed.is_contiguous()
            e_hard = None
        else:
            e_soft = e_soft.to(torch.float32).contiguous()
            e_hard = e_hard.to(torch.float32).contiguous() if want_target else None
        z = torch.empty_like(x, dtype=out_dtype or x.dtype)
        target = torch.empty(R, device=dev, dtype=torch.int64) if want_target else None
        stats = torch.empty(R, 4, device=dev, dtype=torch.float32)
        _lib.check(_lib.lib().focus_gumbel_fwd(_p(x), _p(e_soft) if e_soft is not None else None,
                                               _p(e_hard) if e_hard is not None else None,
                                               _p(seed) if gen else None, _p(z),
                                               _p(target) if target is not None else None, _p(stats), R, V, float(tau),
                                               int(bool(hard)), _dt(x), _dt(z), _stream()), "gumbel_fwd")
        ctx.save_for_backward(x, stats, *([seed] if gen else [e_soft]))
        ctx.gen, ctx.tau, ctx.zdtype = gen, float(tau), z.dtype
        if target is None:
            return z, None
        ctx.mark_non_differentiable(target)
        return z, target

    @staticmethod
    def backward(ctx, dz, _dtarget):
        x, stats, noise = ctx.saved_tensors
        dz = dz.contiguous()
        if dz.dtype != ctx.zdtype:
            dz = dz.to(ctx.zdtype)
        dx = torch.empty_like(x)
        _lib.check(_lib.lib().focus_gumbel_bwd(_p(x), None if ctx.gen else _p(noise), _p(noise) if ctx.gen else None,
                                               _p(stats), _p(dz), _p(dx), x.shape[0], x.shape[1], ctx.tau, _dt(x), _dt(dz), _stream()),
                   "gumbel_bwd")
        return dx, None, None, None, None, None, None, None


def gumbel_softmax_rows(x, tau, hard, e_soft=None, e_hard=None, want_target=True, seed=None, out_dtype=None):
    """x [R, V] raw logits (rows_ok) -> (z [R, V] in x's dtype -- or bf16 from fp32 logits with out_dtype --, target [R] int64
    or None).

    z = gumbel_softmax(log_softmax(x), tau, hard) of STEVE/utils.py:47-61; target = the arg-max of the reference's second,
    hard sample (steve.py:268-269), which is the arg-max of log_softmax(x) + G_hard.  e_soft / e_hard: the Exp(1) draws
    (both given, e.g. the reference's own in a parity test) or None: drawn in the kernel, regenerated by the backward, from
    `seed` (int32 [4] on the device: two words per stream; default: drawn from torch's generator)."""
    assert (e_soft is None) == (e_hard is None) or not want_target, "pass both noise tensors or neither"
    return _GumbelFn.apply(x, tau, hard, e_soft, e_hard, want_target, seed, out_dtype)



# --------------------------------------------------------------------------------------------------
# Slot attention
# --------------------------------------------------------------------------------------------------
class SlotKVGrad:
    """Shared gradient state for the k_t / v_t of ONE frame.  The corrector iterations of a frame all read the same k_t,
    v_t (steve.py:68-83); autograd would sum their three 50 MB gradients with separate add kernels (96 adds per BASELINE
    step).  Iterations that carry the same SlotKVGrad hand autograd ONE gradient, from the node whose backward runs
    last (the others return None) -- valid because every iteration of a frame is on the path to the loss (the slots
    chain through them).  bf16 / K <= 16 / <= 4 iterations: the per-iteration backward only writes its 64-byte
    (w, dlogits) rows and the last node forms dk, dv for all iterations with one MFMA kernel (focus_slot_kv_grad);
    otherwise the backward kernels add into one buffer (focus_slot_attn_bwd accumulate=1)."""

    def __init__(self):
        self.dk = self.dv = None
        self.pending = 0
        self.total = 0
        self.items = []              # deferred mode: (wl, q, dupd) per iteration


class _SlotAttnFn(torch.autograd.Function):
    """One corrector iteration of steve.py:76-83 on one frame.  k_t, v_t [B,N,D]; q [B,K,D]."""

    @staticmethod
    def forward(ctx, k_t, v_t, q, eps, acc):
        _need_gpu(k_t, v_t, q)
        k_t, v_t, q = k_t.contiguous(), v_t.contiguous(), q.contiguous()
        B, N, D = k_t.shape
        K = q.shape[1]
        dev, dt = k_t.device, k_t.dtype
        attn = torch.empty(B, N, K, device=dev, dtype=dt)
        upd = torch.empty(B, K, D, device=dev, dtype=dt)
        cs = torch.empty(B, K, device=dev, dtype=torch.float32)
        L = _lib.lib()
        nb = L.focus_slot_attn_workspace_bytes(B, N, K, D)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        _lib.check(L.focus_slot_attn_fwd(_p(k_t), _p(v_t), N * D, _p(q), _p(attn), N * K, _p(upd), _p(cs), _p(ws), nb,
                                         B, N, K, D, eps, _dt(k_t), _stream()), "slot_attn_fwd")
        ctx.save_for_backward(k_t, v_t, q, attn, cs, upd)
        ctx.eps = eps
        ctx.acc = acc
        if acc is not None:
            acc.pending += 1
            acc.total += 1
        return upd, attn

    @staticmethod
    def backward(ctx, dupd, dattn):
        k_t, v_t, q, attn, cs, upd = ctx.saved_tensors
        B, N, D = k_t.shape
        K = q.shape[1]
        dupd = dupd.contiguous()
        dattn = dattn.contiguous() if dattn is not None else None
        acc = ctx.acc
        L = _lib.lib()
        nb = L.focus_slot_attn_workspace_bytes(B, N, K, D)
        ws = torch.empty(nb, device=k_t.device, dtype=torch.uint8)
        dq = torch.empty_like(q)
        if acc is not None:
            _guard_shared(acc, "slot_attn_step")
        if acc is not None and L.focus_slot_kv_grad_ok(K, D, _dt(k_t), acc.total):
            # deferred: this launch writes its (w, dlogits) rows; the frame's last node forms dk, dv for all iterations
            wl = torch.empty(B, N, 32, device=k_t.device, dtype=k_t.dtype)
            _lib.check(L.focus_slot_attn_bwd(_p(k_t), _p(v_t), N * D, _p(q), _p(attn), N * K, _p(cs), _p(upd), _p(dupd),
                                             _p(dattn), None, None, 0, _p(dq), _p(ws), nb, B, N, K, D, ctx.eps,
                                             _dt(k_t), _p(wl), _stream()), "slot_attn_bwd")
            acc.items.append((wl, q, dupd))
            acc.pending -= 1
            if acc.pending > 0:
                return None, None, dq, None, None
            it = acc.items + [(None, None, None)] * (4 - len(acc.items))
            # one [B,N,2D] matrix [dk | dv]: the projections' backward (linear_kv) then runs one product per gradient
            dkv = torch.empty(B, N, 2 * D, device=k_t.device, dtype=k_t.dtype)
            dk, dv = dkv[..., :D], dkv[..., D:]
            _lib.check(L.focus_slot_kv_grad(*[_p(e[0]) for e in it], *[_p(e[1]) for e in it], *[_p(e[2]) for e in it],
                                            len(acc.items), _p(dk), _p(dv), N * 2 * D, 2 * D, B, N, K, D, _dt(k_t),
                                            _stream()), "slot_kv_grad")
            acc.items = []
            acc.total = 0
            return dk, dv, dq, None, None
        accumulate = 0
        if acc is not None and acc.dk is not None:
            dk, dv, accumulate = acc.dk, acc.dv, 1
        else:
            dk, dv = torch.empty_like(k_t), torch.empty_like(v_t)
            if acc is not None:
                acc.dk, acc.dv = dk, dv
        _lib.check(L.focus_slot_attn_bwd(_p(k_t), _p(v_t), N * D, _p(q), _p(attn), N * K, _p(cs), _p(upd), _p(dupd),
                                         _p(dattn), _p(dk), _p(dv), accumulate, _p(dq), _p(ws), nb, B, N, K, D, ctx.eps,
                                         _dt(k_t), None, _stream()), "slot_attn_bwd")
        if acc is not None:
            acc.pending -= 1
            if acc.pending > 0:
                return None, None, dq, None, None                 # the sum leaves with the last iteration's node
            acc.dk = acc.dv = None
            acc.total = 0
        return dk, dv, dq, None, None


def slot_attn_step(k_t, v_t, q, eps, acc=None):
    """-> (updates [B,K,D], attn_vis [B,N,K]).  acc: a SlotKVGrad shared by the iterations of one frame (optional)."""
    return _SlotAttnFn.apply(k_t, v_t, q, eps, acc)


class _GruGatesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gi, gh, h):
        _need_gpu(gi, gh, h)
        gi, gh, h = gi.contiguous(), gh.contiguous(), h.contiguous()
        R, D = h.shape
        hn = torch.empty_like(h)
        _lib.check(_lib.lib().focus_gru_gates_fwd(_p(gi), _p(gh), _p(h), _p(hn), None, None, R, D, _dt(h), _stream()),
                   "gru_fwd")
        ctx.save_for_backward(gi, gh, h)
        return hn

    @staticmethod
    def backward(ctx, dhn):
        gi, gh, h = ctx.saved_tensors
        R, D = h.shape
        dhn = dhn.contiguous()
        dgi, dgh, dh = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)
        _lib.check(_lib.lib().focus_gru_gates_bwd(_p(gi), _p(gh), _p(h), _p(dhn), _p(dgi), _p(dgh), _p(dh), None, R, D,
                                                  _dt(h), _stream()), "gru_bwd")
        return dgi, dgh, dh


def _stacked_cat(ws, dtype, transposed):
    """The bf16 shadows of several [C, Cin] weights concatenated into one NT-GEMM B operand: rows stacked [sum C, Cin]
    (forward), or the transposes side by side [Cin, sum C] (d(input)); cached like the shadows themselves."""
    def build(out):
        parts = [shadow(w, dtype, transposed=transposed) for w in ws]
        dim = 1 if transposed else 0
        return torch.cat(parts, dim=dim, out=out) if out is not None else torch.cat(parts, dim=dim).contiguous()
    return _stacked_get(tuple(id(w) for w in ws) + (dtype, transposed, "cat"), tuple(ws), None, build)


class _LinearQKVFn(torch.autograd.Function):
    """Three bias-free Linears of one input (transformer.py:33-35, self-attention) as ONE product: the outputs are the
    column blocks of a [rows, 3C] matrix (strided views; ops.small_attention reads them in place and returns its three
    gradients as the blocks of one matrix again), so d(input) = [dq|dk|dv] . [Wq;Wk;Wv] is one product too."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv):
        _need_gpu(x, wq)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        C = wq.shape[0]
        y = mm_nt(x2, _stacked_cat((wq, wk, wv), x.dtype, False)).view(*shp[:-1], 3 * C)
        ctx.save_for_backward(x2, wq, wk, wv)
        ctx.shp = shp
        ds = [_defer_open("linear", (w, None), x2.shape[0], ctx.needs_input_grad[1 + i]) for i, w in enumerate((wq, wk, wv))]
        if any(d is None for d in ds):
            for d in ds:
                if d is not None:
                    d.pending -= 1
            ds = None
        ctx.defer = ds
        return y[..., :C], y[..., C:2 * C], y[..., 2 * C:]

    @staticmethod
    def backward(ctx, dq, dk, dv):
        x2, wq, wk, wv = ctx.saved_tensors
        C = wq.shape[0]
        ds = [t.reshape(-1, C) for t in (dq, dk, dv)]
        es = ds[0].element_size()
        joint = (all(t.stride() == (3 * C, 1) for t in ds) and ds[1].data_ptr() == ds[0].data_ptr() + C * es
                 and ds[2].data_ptr() == ds[1].data_ptr() + C * es and ds[0].dtype == torch.bfloat16 and C % 64 == 0)
        if joint:
            dy = torch.as_strided(ds[0], (ds[0].shape[0], 3 * C), (3 * C, 1))
            dx = mm_nt(dy, _stacked_cat((wq, wk, wv), dy.dtype, True))
        else:
            ds = [t if t.is_contiguous() else t.contiguous() for t in ds]
            dx = _dx_from(ds[0], wq, ds[0].dtype)
            for t, w in ((ds[1], wk), (ds[2], wv)):
                dx = dx + _dx_from(t, w, t.dtype)
        dws = [None, None, None]
        for i, (t, w) in enumerate(zip(ds, (wq, wk, wv))):
            if ctx.defer:
                done = _defer_close(ctx.defer[i], (t, x2))
                if done is not None:
                    dws[i] = done[0]
            else:
                dws[i] = linear_wgrad(t if t.stride(0) % 8 == 0 else t.contiguous(), x2, False)[0]
        return dx.reshape(ctx.shp), dws[0], dws[1], dws[2]


def linear_qkv(x, wq, wk, wv):
    """(x.wq^T, x.wk^T, x.wv^T) as the column blocks of one product (strided views of a [..., 3C] tensor)."""
    return _LinearQKVFn.apply(x, wq, wk, wv)


def _stacked_pair(wa, wb, dtype, transposed):
    """The bf16 shadows of two equally shaped weights as one [2, ...] tensor (the B operands of a batch-2 product);
    cached like the shadows themselves (version, storage, shadow generation)."""
    def build(out):
        parts = [shadow(wa, dtype, transposed=transposed), shadow(wb, dtype, transposed=transposed)]
        return torch.stack(parts, 0, out=out) if out is not None else torch.stack(parts, 0).contiguous()
    return _stacked_get((id(wa), id(wb), dtype, transposed), (wa, wb), None, build)


class _GruCellFn(torch.autograd.Function):
    """nn.GRUCell (STEVE/utils.py:107-118) with its two Linear products as ONE batch-2 launch each way: forward
    [gi | gh] = [x | h] . [W_ih | W_hh]^T (the operands of the two halves are separate tensors: the batch stride of A is
    simply their distance), backward [dx | dh] = [dgi | dgh] . [W_ih | W_hh] + [0 | dhn z].  The gate kernel adds the
    biases.  Per application: 2 launches forward, 2 backward (5 and 7 before, with autograd's accumulation add)."""

    @staticmethod
    def forward(ctx, x, h, w_ih, w_hh, b_ih, b_hh):
        R, D = h.shape
        G = 3 * D
        g = torch.empty(2, R, G, device=x.device, dtype=x.dtype)
        gemm(R, G, D, (x, 0), (D, 1, 0, (h.data_ptr() - x.data_ptr()) // x.element_size()),
             (_stacked_pair(w_ih, w_hh, x.dtype, False), 0), (1, D, 0, G * D), (g, 0), (G, 1, 0, R * G), batch=(1, 2))
        hn = torch.empty_like(h)
        _lib.check(_lib.lib().focus_gru_gates_fwd(_p(g[0]), _p(g[1]), _p(h), _p(hn), _p(b_ih), _p(b_hh), R, D, _dt(h),
                                                  _stream()), "gru_fwd")
        ctx.save_for_backward(x, h, g, w_ih, w_hh, b_ih, b_hh)
        di = _defer_open("linear", (w_ih, b_ih), R, ctx.needs_input_grad[2])
        dh = _defer_open("linear", (w_hh, b_hh), R, ctx.needs_input_grad[3]) if di is not None else None
        if di is not None and dh is None:
            di.pending -= 1
            di = None
        ctx.defer = (di, dh) if di is not None else None
        return hn

    @staticmethod
    def backward(ctx, dhn):
        x, h, g, w_ih, w_hh, b_ih, b_hh = ctx.saved_tensors
        R, D = h.shape
        G = 3 * D
        dhn = dhn.contiguous()
        dg = torch.empty_like(g)
        res = torch.empty(2, R, D, device=h.device, dtype=h.dtype)
        _lib.check(_lib.lib().focus_gru_gates_bwd(_p(g[0]), _p(g[1]), _p(h), _p(dhn), _p(dg[0]), _p(dg[1]), _p(res[1]),
                                                  _p(res[0]), R, D, _dt(h), _stream()), "gru_bwd")
        dxh = torch.empty_like(res)
        gemm(R, D, G, (dg, 0), (G, 1, 0, R * G), (_stacked_pair(w_ih, w_hh, h.dtype, True), 0), (1, G, 0, D * G),
             (dxh, 0), (D, 1, 0, R * D), batch=(1, 2), residual=(res, 0))
        dws = [None, None, None, None]
        if ctx.defer:
            done = _defer_close(ctx.defer[0], (dg[0], x))
            if done is not None:
                dws[0], dws[2] = done
            done = _defer_close(ctx.defer[1], (dg[1], h))
            if done is not None:
                dws[1], dws[3] = done
        else:
            dws[0], dws[2] = linear_wgrad(dg[0], x, True)
            dws[1], dws[3] = linear_wgrad(dg[1], h, True)
        return dxh[0], dxh[1], dws[0], dws[1], dws[2], dws[3]


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh):
    """nn.GRUCell.  x, h [R,D].  bf16 with equal input and hidden widths (the slot update): _GruCellFn; otherwise two
    Linear GEMMs + the gate kernel."""
    if (x.dtype == torch.bfloat16 and x.shape == h.shape and x.is_contiguous() and h.is_contiguous() and x.shape[1] % 32 == 0
            and b_ih is not None and b_hh is not None and (h.data_ptr() - x.data_ptr()) % 16 == 0 and x.is_cuda):
        return _GruCellFn.apply(x, h, w_ih, w_hh, b_ih, b_hh)
    return _GruGatesFn.apply(linear(x, w_ih, b_ih), linear(h, w_hh, b_hh), h)


# --------------------------------------------------------------------------------------------------
# The per-iteration tail of the slot update as one forward launch (csrc/slot_tail.hip):
#   [gru] hn = GRUCell(upd, h)   [mlp] s = hn + W2 relu(W1 LN1(hn) + b1) + b2   [q] q = Wq LN2(slots)
# --------------------------------------------------------------------------------------------------
class SlotTailParams:
    """The parameters of SlotAttentionVideo's recurrent tail (steve.py:35-49), in the order _SlotTailFn takes them."""

    def __init__(self, gru, norm_mlp, mlp, norm_slots, project_q):
        self.tensors = (gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh, norm_mlp.weight, norm_mlp.bias,
                        mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, norm_slots.weight, norm_slots.bias,
                        project_q.weight)
        self.eps = (norm_mlp.eps, norm_slots.eps)


def slot_tail_ok(x, params):
    """The fused tail takes bf16 rows of width 192 with a 768-wide MLP (the BASELINE shape); FOCUS_SLOT_TAIL=0 disables it."""
    if _os.environ.get("FOCUS_SLOT_TAIL", "1") == "0" or x.dtype != torch.bfloat16 or not x.is_cuda:
        return False
    D, H = params.tensors[0].shape[1], params.tensors[6].shape[0]
    return bool(_lib.lib().focus_slot_tail_ok(D, H, BF16)) and all(t is not None for t in params.tensors)


def _tail_wgrad(stash, w, has_b, dy, x):
    """(dw, db) of one Linear application inside the tail: deferred (stacked over the applications) when a stash is open."""
    if stash is not None:
        done = _defer_close(stash, (dy, x))
        return done if done is not None else (None, None)
    return linear_wgrad(dy, x, bool(has_b))


class _SlotTailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, upd, h, eps1, eps2, do_gru, do_mlp, do_q, w_ih, w_hh, b_ih, b_hh, g1, be1, w1, b1, w2, b2, g2, be2, wq):
        _need_gpu(h, wq)
        h = h.contiguous()
        R, D = h.shape
        H = w1.shape[0]
        dev, dt = h.device, h.dtype
        a = _lib.SlotTailArgs()
        a.R, a.D, a.H, a.do_gru, a.do_mlp, a.do_q = R, D, H, int(do_gru), int(do_mlp), int(do_q)
        a.ln1_eps, a.ln2_eps = eps1, eps2
        keep = [h]
        new = lambda *s, dtype=dt: torch.empty(*s, device=dev, dtype=dtype)
        a.h = h.data_ptr()
        sv = {}
        if do_gru:
            upd = upd.contiguous()
            keep.append(upd)
            a.upd = upd.data_ptr()
            ws = [shadow(w_ih, dt), shadow(w_hh, dt)]
            keep += ws
            a.w_ih, a.w_hh, a.b_ih, a.b_hh = ws[0].data_ptr(), ws[1].data_ptr(), b_ih.data_ptr(), b_hh.data_ptr()
            sv["g"], sv["hn"] = new(2, R, 3 * D), new(R, D)
            a.g, a.hn = sv["g"].data_ptr(), sv["hn"].data_ptr()
        if do_mlp:
            ws = [shadow(w1, dt), shadow(w2, dt)]
            keep += ws
            a.ln1_g, a.ln1_b, a.w1, a.b1, a.w2, a.b2 = (g1.data_ptr(), be1.data_ptr(), ws[0].data_ptr(), b1.data_ptr(),
                                                        ws[1].data_ptr(), b2.data_ptr())
            sv["y"], sv["a"], sv["s"] = new(R, D), new(R, H), new(R, D)
            sv["mean1"], sv["rstd1"] = new(R, dtype=torch.float32), new(R, dtype=torch.float32)
            a.y, a.a, a.s, a.mean1, a.rstd1 = (sv["y"].data_ptr(), sv["a"].data_ptr(), sv["s"].data_ptr(), sv["mean1"].data_ptr(),
                                               sv["rstd1"].data_ptr())
        if do_q:
            wqs = shadow(wq, dt)
            keep.append(wqs)
            a.ln2_g, a.ln2_b, a.wq = g2.data_ptr(), be2.data_ptr(), wqs.data_ptr()
            sv["sn"], sv["q"] = new(R, D), new(R, D)
            sv["mean2"], sv["rstd2"] = new(R, dtype=torch.float32), new(R, dtype=torch.float32)
            a.sn, a.q, a.mean2, a.rstd2 = sv["sn"].data_ptr(), sv["q"].data_ptr(), sv["mean2"].data_ptr(), sv["rstd2"].data_ptr()
        _lib.check(_lib.lib().focus_slot_tail_fwd(ctypes.byref(a), _stream()), "slot_tail_fwd")
        out = sv["s"] if do_mlp else (sv["hn"] if do_gru else h.view_as(h))
        ctx.flags = (do_gru, do_mlp, do_q)
        ctx.names = [k for k in ("g", "hn", "y", "a", "s", "mean1", "rstd1", "sn", "mean2", "rstd2") if k in sv]
        ctx.save_for_backward(upd if do_gru else None, h, w_ih, w_hh, g1, w1, w2, g2, wq, *[sv[k] for k in ctx.names])
        ctx.has_b = (b_ih is not None, b1 is not None, b2 is not None)
        ni = ctx.needs_input_grad
        # parameter gradients: stacked over all applications of the slot loop when ops.deferred_wgrads is open
        ctx.st = {}
        if do_gru:
            ctx.st["ih"] = _defer_open("linear", (w_ih, b_ih), R, ni[7])
            ctx.st["hh"] = _defer_open("linear", (w_hh, b_hh), R, ni[8])
        if do_mlp:
            ctx.st["ln1"] = _defer_open("ln", (g1, be1), R, ni[11])
            ctx.st["w1"] = _defer_open("linear", (w1, b1), R, ni[13])
            ctx.st["w2"] = _defer_open("linear", (w2, b2), R, ni[15])
        if do_q:
            ctx.st["ln2"] = _defer_open("ln", (g2, be2), R, ni[17])
            ctx.st["wq"] = _defer_open("linear", (wq, None), R, ni[19])
        return out, (sv["q"] if do_q else None)

    @staticmethod
    def backward(ctx, dout, dq):
        do_gru, do_mlp, do_q = ctx.flags
        saved = ctx.saved_tensors
        upd, h, w_ih, w_hh, g1, w1, w2, g2, wq = saved[:9]
        sv = dict(zip(ctx.names, saved[9:]))
        R, D = h.shape
        dt = h.dtype
        L = _lib.lib()
        grads = {}

        def ln_bwd(dy, x, gamma, mean, rstd, dres, key):
            nblk = L.focus_layernorm_bwd_blocks(R)
            partial = torch.empty(2, nblk, D, device=h.device, dtype=torch.float32)
            dx = torch.empty_like(x)
            st = ctx.st.get(key)
            dg = db = None
            if st is None:
                dg, db = torch.empty(D, device=h.device, dtype=torch.float32), torch.empty(D, device=h.device, dtype=torch.float32)
            _lib.check(L.focus_layernorm_bwd(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres) if dres is not None else None,
                                             _p(dx), _p(dg) if dg is not None else None, _p(db) if db is not None else None,
                                             _p(partial), R, D, _dt(x), _stream()), "layernorm_bwd")
            if st is not None:
                done = _defer_close(st, partial)
                dg, db = done if done is not None else (None, None)
            return dx, dg, db

        if _SLOT_TAIL_BWD and dt == torch.bfloat16 and bool(L.focus_slot_tail_ok(D, w1.shape[0], _dt(h))) \
                and (do_gru or (do_q and dq is not None)):
            return _SlotTailFn._backward_fused(ctx, dout, dq, upd, h, w_ih, w_hh, g1, w1, w2, g2, wq, sv)
        dcur = dout.contiguous() if dout is not None else None
        if do_q and dq is not None:
            dq = dq.contiguous()
            cur = sv["s"] if do_mlp else (sv["hn"] if do_gru else h)
            dsn = _dx_from(dq, wq, dt)
            grads["wq"] = _tail_wgrad(ctx.st.get("wq"), wq, None, dq, sv["sn"])[0]
            dcur, grads["g2"], grads["be2"] = ln_bwd(dsn, cur, g2, sv["mean2"], sv["rstd2"], dcur, "ln2")
        if dcur is None:
            dcur = torch.zeros_like(h)
        if do_mlp:
            ds = dcur
            grads["w2"], grads["b2"] = _tail_wgrad(ctx.st.get("w2"), w2, ctx.has_b[2], ds, sv["a"])
            dz = _dx_from(ds, w2, dt, aux=sv["a"], epilogue=_DEPI[EPI_RELU])
            grads["w1"], grads["b1"] = _tail_wgrad(ctx.st.get("w1"), w1, ctx.has_b[1], dz, sv["y"])
            dy1 = _dx_from(dz, w1, dt)
            dhn, grads["g1"], grads["be1"] = ln_bwd(dy1, sv["hn"], g1, sv["mean1"], sv["rstd1"], ds, "ln1")
        else:
            dhn = dcur
        dupd = None
        if do_gru:
            g = sv["g"]
            G = 3 * D
            dg = torch.empty_like(g)
            res = torch.empty(2, R, D, device=h.device, dtype=dt)
            _lib.check(L.focus_gru_gates_bwd(_p(g[0]), _p(g[1]), _p(h), _p(dhn), _p(dg[0]), _p(dg[1]), _p(res[1]), _p(res[0]), R, D,
                                             _dt(h), _stream()), "gru_bwd")
            dxh = torch.empty_like(res)
            gemm(R, D, G, (dg, 0), (G, 1, 0, R * G), (_stacked_pair(w_ih, w_hh, dt, True), 0), (1, G, 0, D * G),
                 (dxh, 0), (D, 1, 0, R * D), batch=(1, 2), residual=(res, 0))
            grads["w_ih"], grads["b_ih"] = _tail_wgrad(ctx.st.get("ih"), w_ih, ctx.has_b[0], dg[0], upd)
            grads["w_hh"], grads["b_hh"] = _tail_wgrad(ctx.st.get("hh"), w_hh, ctx.has_b[0], dg[1], h)
            dupd, dh = dxh[0], dxh[1]
        else:
            dh = dhn
        gg = grads.get
        return (dupd, dh, None, None, None, None, None, gg("w_ih"), gg("w_hh"), gg("b_ih"), gg("b_hh"), gg("g1"), gg("be1"), gg("w1"),
                gg("b1"), gg("w2"), gg("b2"), gg("g2"), gg("be2"), gg("wq"))


def _slot_tail_backward_fused(ctx, dout, dq, upd, h, w_ih, w_hh, g1, w1, w2, g2, wq, sv):
    """The backward of the tail as ONE launch (focus_slot_tail_bwd): dX chain in the kernel, the dY rows of every weight gradient
    written out and handed to the (deferred) weight-gradient machinery exactly as the composed backward does."""
    do_gru, do_mlp, do_q = ctx.flags
    do_q = do_q and dq is not None
    R, D = h.shape
    H = w1.shape[0]
    dev, dt = h.device, h.dtype
    L = _lib.lib()
    new = lambda *s_, dtype=dt: torch.empty(*s_, device=dev, dtype=dtype)
    a = _lib.SlotTailBwdArgs()
    a.R, a.D, a.H, a.do_gru, a.do_mlp, a.do_q = R, D, H, int(do_gru), int(do_mlp), int(do_q)
    keep = []
    if dout is not None:
        dout = dout.contiguous()
        a.dout = dout.data_ptr()
    nblk = L.focus_slot_tail_bwd_blocks(R)
    ds = dz = dg = dupd = part1 = part2 = None
    dh = new(R, D)
    a.dh, a.h = dh.data_ptr(), h.data_ptr()
    if do_q:
        dq = dq.contiguous()
        cur = sv["s"] if do_mlp else (sv["hn"] if do_gru else h)
        wqt = shadow(wq, dt, transposed=True)
        part2 = new(2, nblk, D, dtype=torch.float32)
        keep += [wqt, cur]
        a.dq, a.cur, a.mean2, a.rstd2, a.ln2_g, a.wq_t, a.part2 = (dq.data_ptr(), cur.data_ptr(), sv["mean2"].data_ptr(),
                                                                   sv["rstd2"].data_ptr(), g2.data_ptr(), wqt.data_ptr(),
                                                                   part2.data_ptr())
    if do_q or do_mlp:
        ds = new(R, D)
        a.ds = ds.data_ptr()
    if do_mlp:
        w1t, w2t = shadow(w1, dt, transposed=True), shadow(w2, dt, transposed=True)
        dz, part1 = new(R, H), new(2, nblk, D, dtype=torch.float32)
        keep += [w1t, w2t]
        a.a, a.hn, a.mean1, a.rstd1, a.ln1_g, a.w1_t, a.w2_t, a.dz, a.part1 = (
            sv["a"].data_ptr(), sv["hn"].data_ptr(), sv["mean1"].data_ptr(), sv["rstd1"].data_ptr(), g1.data_ptr(), w1t.data_ptr(),
            w2t.data_ptr(), dz.data_ptr(), part1.data_ptr())
    if do_gru:
        wit, wht = shadow(w_ih, dt, transposed=True), shadow(w_hh, dt, transposed=True)
        dg, dupd = new(2, R, 3 * D), new(R, D)
        keep += [wit, wht]
        a.g, a.w_ih_t, a.w_hh_t, a.dg, a.dupd = sv["g"].data_ptr(), wit.data_ptr(), wht.data_ptr(), dg.data_ptr(), dupd.data_ptr()
    # [R, D] scratch between the launches of the staged form: dsn | dy1 | z * dhn
    ws = new(3, R, D)
    keep.append(ws)
    a.ws_dsn, a.ws_dy1, a.ws_res = ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr()
    _lib.check(L.focus_slot_tail_bwd(ctypes.byref(a), _stream()), "slot_tail_bwd")
    grads = {}

    def ln_done(key, part):
        st = ctx.st.get(key)
        if st is not None:
            done = _defer_close(st, part)
            return done if done is not None else (None, None)
        both = part.sum(1)
        return both[0], both[1]

    if do_q:
        grads["wq"] = _tail_wgrad(ctx.st.get("wq"), wq, None, dq, sv["sn"])[0]
        grads["g2"], grads["be2"] = ln_done("ln2", part2)
    if do_mlp:
        grads["w2"], grads["b2"] = _tail_wgrad(ctx.st.get("w2"), w2, ctx.has_b[2], ds, sv["a"])
        grads["w1"], grads["b1"] = _tail_wgrad(ctx.st.get("w1"), w1, ctx.has_b[1], dz, sv["y"])
        grads["g1"], grads["be1"] = ln_done("ln1", part1)
    if do_gru:
        grads["w_ih"], grads["b_ih"] = _tail_wgrad(ctx.st.get("ih"), w_ih, ctx.has_b[0], dg[0], upd)
        grads["w_hh"], grads["b_hh"] = _tail_wgrad(ctx.st.get("hh"), w_hh, ctx.has_b[0], dg[1], h)
    gg = grads.get
    return (dupd, dh, None, None, None, None, None, gg("w_ih"), gg("w_hh"), gg("b_ih"), gg("b_hh"), gg("g1"), gg("be1"), gg("w1"),
            gg("b1"), gg("w2"), gg("b2"), gg("g2"), gg("be2"), gg("wq"))


_SlotTailFn._backward_fused = staticmethod(_slot_tail_backward_fused)
# Measured: neither form of focus_slot_tail_bwd beats the five small launches of the composed backward under
# graph replay -- one workgroup per 16 rows streams 1.1 MB of weights by itself (35 us per call; whole step 17.4 -> 18.7 ms),
# the five right-sized launches (FOCUS_SLOT_TAIL_STAGED=1, the default form) redo the LayerNorm backward per column tile and
# wait on scalar gate loads (16.0 -> 17.0 ms).  Both win only where launches are the cost (eager: 38 -> 35 ms).  Off by default.
_SLOT_TAIL_BWD = _os.environ.get("FOCUS_SLOT_TAIL_BWD", "0") != "0"


def slot_tail(upd, h, params, gru=True, mlp=True, q=True):
    """-> (slots [R,D], q [R,D] or None).  upd, h [R,D] bf16 (upd is ignored without gru); see the section comment."""
    return _SlotTailFn.apply(upd, h, float(params.eps[0]), float(params.eps[1]), bool(gru), bool(mlp), bool(q), *params.tensors)


# --------------------------------------------------------------------------------------------------
# BatchNorm2d and MaxPool2d(3, 2, 1) over channels-last feature maps (csrc/batchnorm.hip): the ResNet-18 trunk of STEVE
# --------------------------------------------------------------------------------------------------
def _nhwc_rows(x, dtype=None):
    """[N,C,H,W] of any memory format -> its [N*H*W, C] row matrix, dense (a view of a channels-last tensor)."""
    C = x.shape[1]
    r = x.permute(0, 2, 3, 1).reshape(-1, C)
    if dtype is not None and r.dtype != dtype:
        r = r.to(dtype)
    return r.contiguous()


def _nchw_view(rows, N, H, W):
    """The [N*H*W, C] row matrix as a channels-last [N,C,H,W] tensor."""
    return rows.view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def _bn_workspace(L, R, C, device):
    return torch.empty(L.focus_bn_workspace_bytes(R, C), device=device, dtype=torch.uint8)


class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, training, momentum, eps, relu):
        N, C, H, W = x.shape
        x2 = _nhwc_rows(x)
        R = x2.shape[0]
        L = _lib.lib()
        if training:
            # batch statistics; the running buffers are updated in place by the kernel (no host synchronisation)
            mean = torch.empty(C, device=x.device, dtype=torch.float32)
            rstd = torch.empty(C, device=x.device, dtype=torch.float32)
            _lib.check(L.focus_bn_stats(_p(x2), _p(mean), _p(rstd), _p(running_mean), _p(running_var),
                                        _p(_bn_workspace(L, R, C, x.device)), R, C, eps, momentum, _dt(x2), _stream()),
                       "bn_stats")
        else:
            mean, rstd = running_mean, torch.rsqrt(running_var + eps)
        r2 = None if residual is None else _nhwc_rows(residual, x2.dtype)
        y2 = torch.empty_like(x2)
        _lib.check(L.focus_bn_apply(_p(x2), _p(mean), _p(rstd), _p(weight), _p(bias), _p(r2), _p(y2), R, C, int(relu),
                                    _dt(x2), _stream()), "bn_apply")
        ctx.save_for_backward(x2, y2 if relu else None, mean, rstd, weight)
        ctx.cfg = (N, H, W, bool(relu), not training, None if residual is None else residual.dtype)
        return _nchw_view(y2, N, H, W)

    @staticmethod
    def backward(ctx, dy):
        x2, y2, mean, rstd, weight = ctx.saved_tensors
        N, H, W, relu, frozen, res_dtype = ctx.cfg
        R, C = x2.shape
        L = _lib.lib()
        dy2 = _nhwc_rows(dy, x2.dtype)
        dx2 = torch.empty_like(x2)
        dres2 = torch.empty_like(x2) if res_dtype is not None else None
        dg = torch.empty(C, device=x2.device, dtype=torch.float32)
        db = torch.empty(C, device=x2.device, dtype=torch.float32)
        _lib.check(L.focus_bn_bwd(_p(dy2), _p(x2), _p(y2), _p(mean), _p(rstd), _p(weight), _p(dx2), _p(dres2), _p(dg), _p(db),
                                  _p(_bn_workspace(L, R, C, x2.device)), R, C, int(relu), int(frozen), _dt(x2), _stream()),
                   "bn_bwd")
        dres = None if dres2 is None else _nchw_view(dres2, N, H, W).to(res_dtype)
        return _nchw_view(dx2, N, H, W), dg, db, dres, None, None, None, None, None, None


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum, eps, relu=False, residual=None):
    """nn.BatchNorm2d on the HIP kernels: act(BN(x) [+ residual]) -> channels-last [N,C,H,W] in x's type (fp32 or bf16; the
    parameters and statistics are fp32).  training: batch statistics, running_mean / running_var (None: not tracked) updated
    in place with `momentum`; else the running buffers normalise.  C % 8 == 0, C <= 256."""
    _need_gpu(x, weight, bias, residual, running_mean, running_var)
    if x.dim() != 4:
        raise RuntimeError("focus_amd: batch_norm takes [N,C,H,W] (got %d dimensions)" % x.dim())
    if momentum is None:
        raise RuntimeError("focus_amd: batch_norm with momentum=None (cumulative moving average) is not built")
    if (running_mean is None) != (running_var is None) or (not training and running_mean is None):
        raise RuntimeError("focus_amd: batch_norm needs both running buffers (or, in training mode, neither)")
    for t in (weight, bias, running_mean, running_var):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError("focus_amd: batch_norm parameters and statistics are dense fp32 vectors")
    return _BatchNormFn.apply(x, weight, bias, residual, running_mean, running_var, bool(training), float(momentum),
                              float(eps), bool(relu))


class _MaxPool3x3S2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x2 = _nhwc_rows(x)
        y2 = torch.empty(N * OH * OW, C, device=x.device, dtype=x2.dtype)
        idx = torch.empty(N * OH * OW, C, device=x.device, dtype=torch.int8)
        _lib.check(_lib.lib().focus_maxpool_fwd(_p(x2), _p(y2), _p(idx), N, H, W, C, _dt(x2), _stream()), "maxpool_fwd")
        ctx.save_for_backward(idx)
        ctx.cfg = (N, H, W)
        return _nchw_view(y2, N, OH, OW)

    @staticmethod
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        N, H, W = ctx.cfg
        dy2 = _nhwc_rows(dy)
        C = dy2.shape[1]
        dx2 = torch.empty(N * H * W, C, device=dy.device, dtype=dy2.dtype)
        _lib.check(_lib.lib().focus_maxpool_bwd(_p(dy2), _p(idx), _p(dx2), N, H, W, C, _dt(dy2), _stream()), "maxpool_bwd")
        return _nchw_view(dx2, N, H, W)


def max_pool_3x3_s2(x):
    """nn.MaxPool2d(3, 2, 1) on [N,C,H,W] of any memory format -> channels-last; ties go to the first maximum of the window
    in row-major order, as in ATen.  C % 8 == 0, C <= 256."""
    _need_gpu(x)
    if x.dim() != 4:
        raise RuntimeError("focus_amd: max_pool_3x3_s2 takes [N,C,H,W] (got %d dimensions)" % x.dim())
    return _MaxPool3x3S2Fn.apply(x)


# --------------------------------------------------------------------------------------------------
# clip sampling: decoded uint8 clips -> model inputs (clip_sample.hip)
# --------------------------------------------------------------------------------------------------
CLIP_ITEM_INTS = ("H", "W", "sy0", "sx0", "sh", "sw", "rh", "rw", "oy0", "ox0", "flip")     # focus_clip_item after the pointer and strides


def clip_items(clips, params, out_h, out_w):
    """The host image of the focus_clip_item table of one launch: int64 [n, 9] (pointer, row and frame strides in bytes, then
    the twelve int32 fields in pairs).  clips: uint8 CUDA tensors [T,H,W,3] with dense pixels (strides (*, *, 3, 1)) and one T;
    params: one mapping per clip with sy0, sx0, sh, sw, rh, rw, oy0, ox0, flip.  A rectangle that leaves its frame, an empty
    rectangle or virtual size, or a window that leaves the virtual image is a ValueError: the kernel cannot report it."""
    import numpy as np
    if len(clips) != len(params) or not clips:
        raise ValueError("focus_amd: clip_sample takes one parameter set per clip and at least one clip")
    _need_gpu(*clips)
    T = clips[0].shape[0]
    rec = np.zeros((len(clips), 9), dtype=np.int64)
    for i, (c, p) in enumerate(zip(clips, params)):
        if c.dtype != torch.uint8 or c.dim() != 4 or c.shape[3] != 3 or c.shape[0] != T or (c.numel() and c.stride()[2:] != (3, 1)):
            raise ValueError("focus_amd: clip %d is not a uint8 [T,H,W,3] tensor with dense pixels and T = %d" % (i, T))
        if c.device != clips[0].device:
            raise ValueError("focus_amd: the clips of one launch live on one device")
        H, W = int(c.shape[1]), int(c.shape[2])
        v = dict(H=H, W=W, **{k: int(p[k]) for k in CLIP_ITEM_INTS[2:]})
        v["flip"] = int(bool(p["flip"]))
        if not (v["sh"] >= 1 and v["sw"] >= 1 and 0 <= v["sy0"] and v["sy0"] + v["sh"] <= H and 0 <= v["sx0"] and v["sx0"] + v["sw"] <= W):
            raise ValueError("focus_amd: clip %d: source rectangle (y %d, x %d, h %d, w %d) is outside the %dx%d frame" % (
                i, v["sy0"], v["sx0"], v["sh"], v["sw"], H, W))
        if not (v["rh"] >= 1 and v["rw"] >= 1 and 0 <= v["oy0"] and v["oy0"] + out_h <= v["rh"] and 0 <= v["ox0"]
                and v["ox0"] + out_w <= v["rw"]):
            raise ValueError("focus_amd: clip %d: the %dx%d window at (%d, %d) is outside the resized %dx%d image" % (
                i, out_h, out_w, v["oy0"], v["ox0"], v["rh"], v["rw"]))
        rec[i, 0], rec[i, 1], rec[i, 2] = c.data_ptr(), c.stride(1), c.stride(0)
        ints = [v[k] for k in CLIP_ITEM_INTS] + [0]
        for k in range(6):
            rec[i, 3 + k] = ints[2 * k] | (ints[2 * k + 1] << 32)
    return rec


def clip_sample(clips, params, out_h, out_w, mean, std, reverse=False, dtype=torch.float32, layout="BCTHW"):
    """Decoded clips -> model inputs in ONE launch: per clip, crop the rectangle, resize it bilinearly (align_corners=False)
    to (rh, rw), take the out_h x out_w window at (oy0, ox0), mirror it when flip, normalise (v/255 - mean) / std, reverse
    the channels (after normalisation, as pack_pathway_output does) and cast.  layout "BCTHW" (Motionformer) or "BTCHW"
    (STEVE).  One small H2D copy carries the descriptor table.  No CPU fallback."""
    if layout not in ("BCTHW", "BTCHW"):
        raise ValueError("focus_amd: clip_sample layout is BCTHW or BTCHW (got %r)" % (layout,))
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("focus_amd: unsupported dtype %s (float32 or bfloat16)" % dtype)
    if out_h < 1 or out_w < 1:
        raise ValueError("focus_amd: clip_sample output size %dx%d" % (out_h, out_w))
    if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
        raise ValueError("focus_amd: clip_sample takes three means and three non-zero stds")
    rec = clip_items(clips, params, out_h, out_w)
    dev, B, T = clips[0].device, len(clips), int(clips[0].shape[0])
    plane = out_h * out_w
    if layout == "BCTHW":
        out = torch.empty(B, 3, T, out_h, out_w, device=dev, dtype=dtype)
        sc, st = T * plane, plane
    else:
        out = torch.empty(B, T, 3, out_h, out_w, device=dev, dtype=dtype)
        sc, st = plane, 3 * plane
    mean3, std3 = (ctypes.c_float * 3)(*[float(m) for m in mean]), (ctypes.c_float * 3)(*[float(s) for s in std])
    with torch.cuda.device(dev):
        items = torch.from_numpy(rec).pin_memory().to(dev, non_blocking=True)
        _lib.check(_lib.lib().focus_clip_sample(_p(items), B, T, out_h, out_w, _p(out), 3 * T * plane, sc, st,
                                                ctypes.cast(mean3, ctypes.c_void_p), ctypes.cast(std3, ctypes.c_void_p),
                                                int(bool(reverse)), _dt(out), _stream()), "clip_sample")
    return out


# --------------------------------------------------------------------------------------------------
# clip sampling with a colour stage: the AVA front end (clip_color.hip)
# --------------------------------------------------------------------------------------------------
COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION = 0, 1, 2          # enum focus_color_op


def clip_colors(colors, n_clips):
    """The host image of the focus_clip_color table: int32 [n, 10] (n_ops, op[3], then alpha[3] and shift[3] as float bits).
    colors: one mapping per clip with `op` (0..3 kinds of COLOR_*, applied in this order), `alpha` (one weight per op) and
    `shift` (three floats by source channel).  More than three ops, an unknown or repeated kind, or an alpha / shift that is
    not finite is a ValueError: the kernels cannot report it.  Needs no device."""
    import math
    import numpy as np
    if len(colors) != n_clips:
        raise ValueError("focus_amd: clip_sample_color takes one colour record per clip (%d for %d clips)" % (len(colors), n_clips))
    rec = np.zeros((n_clips, 10), dtype=np.int32)
    flt = rec.view(np.float32)
    for i, c in enumerate(colors):
        op, alpha, shift = [int(k) for k in c["op"]], [float(a) for a in c["alpha"]], [float(s) for s in c["shift"]]
        if len(op) > 3 or len(alpha) != len(op):
            raise ValueError("focus_amd: clip %d: %d colour ops with %d weights (at most three, one weight each)" % (i, len(op), len(alpha)))
        if any(k not in (COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION) for k in op) or len(set(op)) != len(op):
            raise ValueError("focus_amd: clip %d: colour ops %r (each of brightness 0, contrast 1, saturation 2 at most once)" % (i, op))
        if len(shift) != 3 or not all(math.isfinite(v) for v in alpha + shift):
            raise ValueError("focus_amd: clip %d: alpha %r / shift %r (finite, three shifts)" % (i, alpha, shift))
        rec[i, 0] = len(op)
        rec[i, 1:1 + len(op)] = op
        flt[i, 4:4 + len(op)] = alpha
        flt[i, 7:10] = shift
    return rec


def clip_sample_color(clips, params, colors, out_h, out_w, mean, std, gray_w, reverse=False, dtype=torch.float32, layout="BCTHW"):
    """clip_sample with the colour stage of the AVA pipeline between /255 and the normalisation: per clip the ops of its
    record (clip_colors) in the record's order -- brightness x*a, saturation x*a + g*(1-a) with g the pixel's grey, contrast
    x*a + m_t*(1-a) with m_t the mean grey of output frame t as it stands when contrast runs -- then + shift, mean / std,
    the reversal and the cast.  gray_w, shift, mean and std go by SOURCE channel.  One pinned H2D copy carries both tables;
    focus_clip_gray_mean runs only when some record holds contrast, then focus_clip_sample_color: at most two launches.
    No CPU fallback."""
    import numpy as np
    if layout not in ("BCTHW", "BTCHW"):
        raise ValueError("focus_amd: clip_sample_color layout is BCTHW or BTCHW (got %r)" % (layout,))
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("focus_amd: unsupported dtype %s (float32 or bfloat16)" % dtype)
    if out_h < 1 or out_w < 1:
        raise ValueError("focus_amd: clip_sample_color output size %dx%d" % (out_h, out_w))
    if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
        raise ValueError("focus_amd: clip_sample_color takes three means and three non-zero stds")
    if len(gray_w) != 3 or not all(np.isfinite(float(w)) for w in gray_w):
        raise ValueError("focus_amd: clip_sample_color takes three finite grey weights")
    if len(clips) != len(params) or not clips:
        raise ValueError("focus_amd: clip_sample_color takes one parameter set per clip and at least one clip")
    col = clip_colors(colors, len(clips))
    rec = clip_items(clips, params, out_h, out_w)
    dev, B, T = clips[0].device, len(clips), int(clips[0].shape[0])
    plane = out_h * out_w
    if layout == "BCTHW":
        out = torch.empty(B, 3, T, out_h, out_w, device=dev, dtype=dtype)
        sc, st = T * plane, plane
    else:
        out = torch.empty(B, T, 3, out_h, out_w, device=dev, dtype=dtype)
        sc, st = plane, 3 * plane
    f3 = lambda v: ctypes.cast((ctypes.c_float * 3)(*[float(x) for x in v]), ctypes.c_void_p)
    keep = [f3(mean), f3(std), f3(gray_w)]
    contrast = bool(((col[:, 1:4] == COLOR_CONTRAST) & (np.arange(3)[None] < col[:, :1])).any())
    table = np.concatenate([rec.view(np.uint8).reshape(-1), col.view(np.uint8).reshape(-1)])      # items (72 B each), then colours
    L = _lib.lib()
    with torch.cuda.device(dev):
        tab = torch.from_numpy(table).pin_memory().to(dev, non_blocking=True)
        items, cols = tab.data_ptr(), tab.data_ptr() + rec.nbytes
        frame_mean = torch.empty(B * T, device=dev, dtype=torch.float32)      # read only for clips with contrast
        if contrast:
            nbytes = int(L.focus_clip_color_workspace_bytes(B, T, out_h, out_w))
            ws = torch.empty(max(nbytes, 4), device=dev, dtype=torch.uint8)
            _lib.check(L.focus_clip_gray_mean(items, cols, B, T, out_h, out_w, keep[2], _p(frame_mean), _p(ws), nbytes, _stream()),
                       "clip_gray_mean")
        _lib.check(L.focus_clip_sample_color(items, cols, _p(frame_mean), B, T, out_h, out_w, _p(out), 3 * T * plane, sc, st,
                                             keep[0], keep[1], keep[2], int(bool(reverse)), _dt(out), _stream()), "clip_sample_color")
    return out


# --------------------------------------------------------------------------------------------------
# Mixup / CutMix on the device (datasets/mixup.py:40-192) and the soft-target loss (losses.py:15-36): csrc/mixup.hip
# --------------------------------------------------------------------------------------------------
def _need_dense(x, what):
    _need_gpu(x)
    if not x.is_contiguous():
        raise ValueError("focus_amd: %s works in place on a contiguous tensor (mixing a copy would leave the "
                         "caller's tensor unmixed); got strides %s for shape %s" % (what, tuple(x.stride()), tuple(x.shape)))


def mixup_blend_(x, lam):
    """x <- x * lam + x.flip(0) * (1 - lam) in place, with the bits of ATen's `x.flip(0).mul_(1 - lam)`,
    `x.mul_(lam).add_(...)` (three separately rounded operations), in one pass and without the flipped copy.
    x: [B, ...] fp32 or bf16, contiguous.  Returns x itself.  No CPU fallback."""
    _need_dense(x, "mixup_blend_")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError("focus_amd: mixup_blend_ needs a non-empty [B, ...] tensor")
    lam = float(lam)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().focus_mixup_blend(_p(x), x.shape[0], x.numel() // x.shape[0], lam, 1.0 - lam, _dt(x),
                                                _stream()), "mixup_blend")
    return x


def cutmix_paste_(x, yl, yh, xl, xh):
    """x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh] in place, as a swap of the rectangle between samples i and
    B-1-i.  x: [B, ..., H, W] fp32 or bf16, contiguous ([B,3,T,H,W] and [B,T,3,H,W] alike).  Returns x itself."""
    _need_dense(x, "cutmix_paste_")
    if x.dim() < 3 or x.numel() == 0:
        raise ValueError("focus_amd: cutmix_paste_ needs a non-empty [B, ..., H, W] tensor")
    yl, yh, xl, xh = int(yl), int(yh), int(xl), int(xh)
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    if not (0 <= yl <= yh <= H and 0 <= xl <= xh <= W):
        raise ValueError("focus_amd: cutmix box y %d:%d x %d:%d outside the %dx%d frame" % (yl, yh, xl, xh, H, W))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().focus_cutmix_paste(_p(x), B, x.numel() // (B * H * W), H, W, yl, yh, xl, xh, _dt(x),
                                                 _stream()), "cutmix_paste")
    return x


def mixup_target(labels, num_classes, lam=1.0, smoothing=0.0):
    """Dense fp32 [B, num_classes] target of mixup.py:40-64 in one launch: smoothed one-hot rows of `labels` and of
    `labels.flip(0)`, mixed with lam / 1 - lam.  labels: [B] integer class indices on the device."""
    _need_gpu(labels)
    num_classes = int(num_classes)
    if labels.dim() != 1 or labels.numel() < 1 or num_classes < 1 or labels.is_floating_point():
        raise ValueError("focus_amd: mixup_target takes [B] integer labels and num_classes >= 1")
    labels = labels.long().contiguous()
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    lam = float(lam)
    target = torch.empty(labels.shape[0], num_classes, device=labels.device, dtype=torch.float32)
    with torch.cuda.device(labels.device):
        _lib.check(_lib.lib().focus_mixup_target(_p(labels), _p(target), labels.shape[0], num_classes, on, off, lam,
                                                 1.0 - lam, _stream()), "mixup_target")
    return target


class _XentSoftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, mean):
        R, V = logits.shape
        x = logits.float().contiguous()
        loss_rows = torch.empty(R, device=logits.device, dtype=torch.float32)
        dlog = torch.empty_like(x)
        _lib.check(_lib.lib().focus_xent_soft(_p(x), _p(target), _p(loss_rows), _p(dlog), R, V, _stream()), "xent_soft")
        ctx.save_for_backward(dlog)
        ctx.mean, ctx.dtype = mean, logits.dtype
        return loss_rows.mean() if mean else loss_rows

    @staticmethod
    def backward(ctx, g):
        (dlog,) = ctx.saved_tensors                 # d(mean over rows) / d(logits)
        g = g.float()
        d = dlog * g if ctx.mean else dlog * (g * dlog.shape[0])[:, None]
        return d.to(ctx.dtype), None, None


def soft_target_ce(logits, target, reduction="mean"):
    """sum(-target * log_softmax(logits), -1) with its gradient from one row kernel; reduction "mean" or "none".
    logits [R,V] fp32 or bf16 (widened first; the gradient comes back in the logits' type), target [R,V] (used as fp32;
    the rows need not sum to 1, no gradient flows into it)."""
    _need_gpu(logits, target)
    if reduction not in ("mean", "none"):
        raise ValueError("focus_amd: soft_target_ce reduction is 'mean' or 'none' (got %r)" % (reduction,))
    if logits.dim() != 2 or logits.shape != target.shape or logits.numel() == 0:
        raise ValueError("focus_amd: soft_target_ce takes logits and target of one [R,V] shape (got %s and %s)" %
                         (tuple(logits.shape), tuple(target.shape)))
    _dt(logits)
    return _XentSoftFn.apply(logits, target.detach().float().contiguous(), reduction == "mean")


# --------------------------------------------------------------------------------------------------
# Random erasing of normalised clips in place (random_erase.hip; the plans come from slowfast/datasets/random_erasing.py)
# --------------------------------------------------------------------------------------------------
ERASE_MODES = ("const", "rand", "pixel")                                   # enum focus_erase_mode
ERASE_ITEM_FIELDS = ("clip", "t0", "t1", "top", "left", "h", "w")         # focus_erase_item, in front of `ord`
ERASE_MAX_PER_CLIP = 64                                                    # FOCUS_ERASE_MAX_PER_CLIP


def erase_table(items, B, T, H, W):
    """The host image of the focus_erase_item table: int32 [n, 8], and the largest number of items one clip has.  items:
    mappings with clip, t0, t1, top, left, h, w; the items of one clip are applied in the order they are listed (a later one
    wins where they overlap) and are made contiguous here.  A rectangle or frame range that is empty or leaves the
    [B, T, H, W] tensor, or more than ERASE_MAX_PER_CLIP items for one clip, is a ValueError: the kernel cannot report it."""
    import numpy as np
    per_clip = {}
    for n, it in enumerate(items):
        try:
            v = [it[k] for k in ERASE_ITEM_FIELDS]
        except (KeyError, TypeError, IndexError):
            raise ValueError("focus_amd: erase item %d is not a mapping with %s" % (n, ", ".join(ERASE_ITEM_FIELDS)))
        if any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in v):
            raise ValueError("focus_amd: erase item %d: %r are not all integers" % (n, v))
        clip, t0, t1, top, left, h, w = (int(a) for a in v)
        if not 0 <= clip < B:
            raise ValueError("focus_amd: erase item %d: clip %d outside the batch of %d" % (n, clip, B))
        if not 0 <= t0 < t1 <= T:
            raise ValueError("focus_amd: erase item %d: frames [%d, %d) are empty or outside the %d frames" % (n, t0, t1, T))
        if not (h >= 1 and w >= 1 and 0 <= top and top + h <= H and 0 <= left and left + w <= W):
            raise ValueError("focus_amd: erase item %d: rectangle (top %d, left %d, h %d, w %d) is empty or outside the "
                             "%dx%d frame" % (n, top, left, h, w, H, W))
        rows = per_clip.setdefault(clip, [])
        rows.append((clip, t0, t1, top, left, h, w, len(rows)))
    most = max((len(r) for r in per_clip.values()), default=0)
    if most > ERASE_MAX_PER_CLIP:
        raise ValueError("focus_amd: %d erase items for one clip (at most %d)" % (most, ERASE_MAX_PER_CLIP))
    rec = np.array([r for clip in sorted(per_clip) for r in per_clip[clip]], dtype=np.int32).reshape(-1, 8)
    if rec.shape[0] > 65535:
        raise ValueError("focus_amd: random_erase_ takes at most 65535 items per call (got %d)" % rec.shape[0])
    return rec, most


def random_erase_(x, items, mode, layout, seed=None):
    """RandomErasing of a batch of clips IN PLACE, one launch: x [B,C,T,H,W] (layout "BCTHW") or [B,T,C,H,W] ("BTCHW"), fp32 or
    bf16, contiguous -- what clip_sample returns.  items: see erase_table (datasets/random_erasing.RandomErasing.plan makes
    them).  mode "const" writes +0.0, "rand" one N(0,1) value per (item, frame, channel), "pixel" one per element, from the
    build-owned generator of include/focus_amd.h; `seed`: int32 [2] on x's device (default: drawn from torch's generator).
    One H2D copy of the table, one launch; an empty item list launches nothing.  Returns x itself.  No CPU fallback."""
    if layout not in ("BCTHW", "BTCHW"):
        raise ValueError("focus_amd: random_erase_ layout is BCTHW or BTCHW (got %r)" % (layout,))
    if mode not in ERASE_MODES:
        raise ValueError("focus_amd: random_erase_ mode is one of %s (got %r)" % (", ".join(ERASE_MODES), mode))
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError("focus_amd: random_erase_ needs a non-empty 5-d tensor (got shape %s)" % (tuple(x.shape),))
    B, H, W = int(x.shape[0]), int(x.shape[3]), int(x.shape[4])
    C, T = (int(x.shape[1]), int(x.shape[2])) if layout == "BCTHW" else (int(x.shape[2]), int(x.shape[1]))
    if H > 32768 or W > 32768 or T > 65535 or C > 65535:
        raise ValueError("focus_amd: random_erase_ takes frames up to 32768 a side and up to 65535 frames and channels")
    rec, most = erase_table(items, B, T, H, W)
    _need_dense(x, "random_erase_")
    dt = _dt(x)
    if seed is not None and (not seed.is_cuda or seed.device != x.device or seed.dtype != torch.int32 or seed.numel() < 2
                             or not seed.is_contiguous()):
        raise ValueError("focus_amd: random_erase_ seed is a contiguous int32 [2] tensor on the clips' device")
    if rec.shape[0] == 0:
        return x
    plane = H * W
    sc, st = (T * plane, plane) if layout == "BCTHW" else (plane, C * plane)
    with torch.cuda.device(x.device):
        if seed is None and mode != "const":
            seed = torch.randint(-2 ** 31, 2 ** 31 - 1, (2,), device=x.device, dtype=torch.int32)
        table = torch.from_numpy(rec).pin_memory().to(x.device, non_blocking=True)
        _lib.check(_lib.lib().focus_random_erase(_p(x), dt, B, T, C, H, W, C * T * plane, sc, st, _p(table), rec.shape[0], most,
                                                 ERASE_MODES.index(mode), _p(seed), _stream()), "random_erase")
    return x


# --------------------------------------------------------------------------------------------------
# RandAugment on device uint8 clips (randaug.hip; the plans come from slowfast/datasets/rand_augment.py)
# --------------------------------------------------------------------------------------------------
RANDAUG_OPS = ("copy", "autocontrast", "equalize", "invert", "posterize", "solarize", "solarize_add", "brightness", "color",
               "contrast", "sharpness", "rotate", "shear_x", "shear_y", "translate_x", "translate_y")   # enum focus_randaug_op
RANDAUG_STAT_OPS, RANDAUG_AFFINE_OPS = (1, 2, 9), (11, 12, 13, 14, 15)
RANDAUG_STAT_WORDS = 776
RANDAUG_RESAMPLES = (2, 3)                  # PIL's BILINEAR, BICUBIC


def _randaug_item_dtype():
    import numpy as np
    return np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_stride", "<i8"), ("dst_stride", "<i8"), ("stats_off", "<i8"),
                     ("coef", "<f8", (6,)), ("farg", "<f4"), ("iarg", "<i4"), ("H", "<i4"), ("W", "<i4"), ("op", "<i4"),
                     ("resample", "<i4"), ("fill", "u1", (4,)), ("pad_", "<i4")])          # focus_randaug_item, 120 bytes


def _randaug_record(r, where):
    """A layer record of a plan, validated -> (op, farg, iarg, fill, resample, coef); a closed gate or PIL's plain copy -> None."""
    import math
    import numpy as np
    if r is None:
        return None
    op = r["op"]
    if isinstance(op, bool) or not isinstance(op, (int, np.integer)) or not 0 <= int(op) < len(RANDAUG_OPS):
        raise ValueError("focus_amd: %s: unknown RandAugment op %r" % (where, op))
    op = int(op)
    fill = tuple(int(v) for v in r.get("fill", (128, 128, 128)))
    if len(fill) != 3 or any(not 0 <= v <= 255 for v in fill):
        raise ValueError("focus_amd: %s: fill %r is not three bytes" % (where, fill))
    rs, coef = 2, (0.0,) * 6
    if op in RANDAUG_AFFINE_OPS:
        rs = r.get("resample", 2)
        rs = rs[0] if isinstance(rs, (tuple, list)) and len(rs) == 1 else rs
        if rs not in RANDAUG_RESAMPLES:
            raise ValueError("focus_amd: %s: resample %r (2 bilinear or 3 bicubic)" % (where, rs))
        coef = r.get("coef")
        if coef is None:                                              # PIL returns a copy (rotation by 0)
            return None
        if len(coef) != 6 or not all(math.isfinite(float(v)) for v in coef):
            raise ValueError("focus_amd: %s: six finite coefficients, got %r" % (where, coef))
        coef = tuple(float(v) for v in coef)
    return op, float(r.get("farg", 0.0)), int(r.get("iarg", 0)), fill, int(rs), coef


def randaug_apply(clips_u8, plans):
    """RandAugment of a batch of decoded clips on the device.  clips_u8: uint8 CUDA tensors [T,H,W,3] with dense pixels (H, W,
    T may differ per clip); plans[i][t]: the layer records of frame t of clip i, as RandAugment.plan returns them for one
    image -- None (the gate stayed closed: the frame is copied) or a mapping with op (a code of RANDAUG_OPS), farg, iarg,
    resample (2 bilinear / 3 bicubic, or a 1-tuple of it), coef (six floats; None: a plain copy) and fill.  Every frame has the
    same number of layers.  Returns NEW tensors of the inputs' shapes; the inputs are not written.  One H2D copy of the
    descriptor table of all layers, then per layer the apply launch and, when a frame of the layer needs its histogram or its
    mean, a stats launch before it.  Everything the kernel cannot report is a ValueError here.  No CPU fallback."""
    import numpy as np
    t = randaug_table(clips_u8, plans)
    rec, n, dev = t["rec"], t["rec"].shape[1], clips_u8[0].device
    L = _lib.lib()
    ws_bytes = int(L.focus_randaug_workspace_bytes(t["n_stats"]))
    with torch.cuda.device(dev):
        ws = torch.zeros(ws_bytes // 4, dtype=torch.int32, device=dev) if t["n_stats"] else None
        items = torch.from_numpy(rec.reshape(-1).view(np.uint8)).pin_memory().to(dev, non_blocking=True)
        for l in range(rec.shape[0]):
            _lib.check(L.focus_randaug_layer(ctypes.c_void_p(items.data_ptr() + l * n * rec.dtype.itemsize), n, t["max_h"],
                                             t["max_w"], int(t["need_stats"][l]), _p(ws), ws_bytes, _stream()), "randaug_layer")
    return t["outs"]


def randaug_table(clips_u8, plans):
    """The host half of randaug_apply: validates, allocates the output and scratch clips and writes the focus_randaug_item
    table of every layer.  -> dict(rec [depth, n] structured array, outs, scratch, n_stats, need_stats [depth], max_h, max_w)."""
    import numpy as np
    if not clips_u8 or len(clips_u8) != len(plans):
        raise ValueError("focus_amd: randaug_apply takes one plan list per clip and at least one clip")
    dev = clips_u8[0].device
    depth = None
    frames = []                                                       # (clip index, t, H, W, validated layers)
    for i, (c, pl) in enumerate(zip(clips_u8, plans)):
        if c.dtype != torch.uint8 or c.dim() != 4 or c.shape[3] != 3 or c.numel() == 0 or c.stride()[2:] != (3, 1):
            raise ValueError("focus_amd: clip %d is not a non-empty uint8 [T,H,W,3] tensor with dense pixels" % i)
        if c.device != dev:
            raise ValueError("focus_amd: the clips of one launch live on one device")
        if c.shape[1] > 32768 or c.shape[2] > 32768:
            raise ValueError("focus_amd: clip %d: frames above 32768 pixels a side are not supported" % i)
        if len(pl) != c.shape[0]:
            raise ValueError("focus_amd: clip %d has %d frames and %d plans" % (i, c.shape[0], len(pl)))
        for t, layers in enumerate(pl):
            depth = len(layers) if depth is None else depth
            if len(layers) != depth or depth < 1:
                raise ValueError("focus_amd: every frame's plan has the same number of layers, at least one "
                                 "(clip %d frame %d: %d, expected %d)" % (i, t, len(layers), depth))
            frames.append((i, t, int(c.shape[1]), int(c.shape[2]),
                           [_randaug_record(r, "clip %d frame %d layer %d" % (i, t, l)) for l, r in enumerate(layers)]))
    n = len(frames)
    if n > 65535:
        raise ValueError("focus_amd: randaug_apply takes at most 65535 frames per call (got %d)" % n)
    if not dev.type == "cuda":
        raise ValueError("focus_amd: randaug_apply runs on the MI355X only (got %s tensors); there is no CPU fallback" % dev)
    outs = [torch.empty(c.shape, dtype=torch.uint8, device=dev) for c in clips_u8]
    scratch = [torch.empty_like(o) for o in outs] if depth > 1 else outs
    rec = np.zeros((depth, n), dtype=_randaug_item_dtype())
    n_stats, need_stats = 0, [False] * depth
    for k, (i, t, H, W, layers) in enumerate(frames):
        for l, r in enumerate(layers):
            # layer l writes `outs` when an even number of layers follows it, so the last one always does
            src = clips_u8[i] if l == 0 else (outs if (depth - l) % 2 == 0 else scratch)[i]
            dst = (outs if (depth - 1 - l) % 2 == 0 else scratch)[i]
            it = rec[l, k]
            it["src"], it["src_stride"] = src.data_ptr() + t * src.stride(0), src.stride(1)
            it["dst"], it["dst_stride"] = dst.data_ptr() + t * dst.stride(0), dst.stride(1)
            it["H"], it["W"], it["stats_off"], it["op"], it["resample"] = H, W, -1, 0, 2
            if r is None:
                continue
            it["op"], it["farg"], it["iarg"], it["resample"], it["coef"] = r[0], r[1], r[2], r[4], r[5]
            it["fill"][:3] = r[3]
            if r[0] in RANDAUG_STAT_OPS:
                it["stats_off"] = n_stats * RANDAUG_STAT_WORDS
                n_stats += 1
                need_stats[l] = True
    return dict(rec=rec, outs=outs, scratch=scratch, n_stats=n_stats, need_stats=need_stats,
                max_h=max(f[2] for f in frames), max_w=max(f[3] for f in frames))


# --------------------------------------------------------------------------------------------------
# Slot masks -> segments, ORViT boxes and FG-ARI tables (csrc/slot_segments.hip)
# --------------------------------------------------------------------------------------------------
def _need_contiguous(t, what):
    if not t.is_contiguous():
        raise ValueError("focus_amd: %s must be contiguous; got strides %s for shape %s" % (
            what, tuple(t.stride()), tuple(t.shape)))


def slot_segments(attn, He, We):
    """attn [B,T,N = He*We,K] (the slot update's attention, fp32 or bf16, contiguous) -> (seg uint8 [B,T,N], the arg-max
    slot of each cell with ties to the lowest index; stats int32 [B,T,K,5] = (count, xmin, ymin, xmax, ymax) per frame and
    slot in cell units, (0, We, He, -1, -1) for a slot without a cell).  No CPU fallback."""
    _need_gpu(attn)
    He, We = int(He), int(We)
    if attn.dim() != 4 or attn.shape[2] != He * We or not 1 <= attn.shape[3] <= 32 or He < 1 or We < 1:
        raise ValueError("focus_amd: slot_segments takes attn [B,T,He*We,K] with 1 <= K <= 32; got %s for a %dx%d grid" % (
            tuple(attn.shape), He, We))
    _need_contiguous(attn, "slot_segments' attn")
    B, T, N, K = attn.shape
    seg = torch.empty(B, T, N, device=attn.device, dtype=torch.uint8)
    stats = torch.empty(B, T, K, 5, device=attn.device, dtype=torch.int32)
    with torch.cuda.device(attn.device):
        _lib.check(_lib.lib().focus_slot_segments(_p(attn), _dt(attn), B, T, He, We, K, _p(seg), _p(stats), _stream()),
                   "slot_segments")
    return seg, stats


def slot_boxes(stats, He, We, H, W, O, drop_largest=True):
    """stats [B,T,K,5] of slot_segments -> (boxes fp32 [B,T,O,4] in the orvit_bboxes encoding, slot_ids int32 [B,O]): per
    clip the O largest slots (after dropping the largest = background when drop_largest), in ascending slot index; missing
    objects are zero rows with id -1.  (H, W) is the frame the boxes refer to; He | H and We | W."""
    _need_gpu(stats)
    He, We, H, W, O = int(He), int(We), int(H), int(W), int(O)
    if stats.dim() != 4 or stats.shape[3] != 5 or stats.dtype != torch.int32 or not 1 <= stats.shape[2] <= 32 or O < 0:
        raise ValueError("focus_amd: slot_boxes takes int32 stats [B,T,K,5] with 1 <= K <= 32 and O >= 0; got %s %s" % (
            stats.dtype, tuple(stats.shape)))
    if He < 1 or We < 1 or H < 1 or W < 1 or H % He or W % We:
        raise ValueError("focus_amd: slot_boxes: the %dx%d slot grid does not divide the %dx%d frame" % (He, We, H, W))
    _need_contiguous(stats, "slot_boxes' stats")
    B, T, K, _ = stats.shape
    boxes = torch.empty(B, T, O, 4, device=stats.device, dtype=torch.float32)
    slot_ids = torch.empty(B, O, device=stats.device, dtype=torch.int32)
    with torch.cuda.device(stats.device):
        _lib.check(_lib.lib().focus_slot_boxes(_p(stats), B, T, K, He, We, H, W, O, int(bool(drop_largest)), _p(boxes),
                                               _p(slot_ids), _stream()), "slot_boxes")
    return boxes, slot_ids


def seg_contingency(seg, truth, He, We, K, first_segment=1):
    """seg uint8 [B,T,He*We] (or [B,T,He,We]) and truth [B,T,S,1,H,W] (bool / uint8 / fp32, non-zero = member) -> the FG-ARI
    contingency tables int32 [B, S - first_segment, K]: pixels of truth segment s (all frames) whose cell belongs to slot k."""
    _need_gpu(seg, truth)
    He, We, K, first_segment = int(He), int(We), int(K), int(first_segment)
    if truth.dtype == torch.bool:
        truth = truth.view(torch.uint8)
    if seg.dtype != torch.uint8 or truth.dtype not in (torch.uint8, torch.float32):
        raise ValueError("focus_amd: seg_contingency takes a uint8 seg and a bool, uint8 or float32 truth; got %s, %s" % (
            seg.dtype, truth.dtype))
    if truth.dim() != 6 or truth.shape[3] != 1 or seg.dim() not in (3, 4) or seg.shape[:2] != truth.shape[:2] \
            or seg.numel() != truth.shape[0] * truth.shape[1] * He * We or seg.device != truth.device:
        raise ValueError("focus_amd: seg_contingency takes seg [B,T,He*We] and truth [B,T,S,1,H,W] on one device; got %s, %s"
                         % (tuple(seg.shape), tuple(truth.shape)))
    B, T, S, _, H, W = truth.shape
    if not 1 <= K <= 32 or He < 1 or We < 1 or H % He or W % We or not 0 <= first_segment < S or T * H * W >= 2 ** 31:
        raise ValueError("focus_amd: seg_contingency: K %d, grid %dx%d, frame %dx%d, S %d, first_segment %d" % (
            K, He, We, H, W, S, first_segment))
    _need_contiguous(seg, "seg_contingency's seg")
    _need_contiguous(truth, "seg_contingency's truth")
    table = torch.empty(B, S - first_segment, K, device=seg.device, dtype=torch.int32)
    with torch.cuda.device(seg.device):
        _lib.check(_lib.lib().focus_seg_contingency(_p(seg), _p(truth), int(truth.dtype == torch.float32), B, T, S, H, W, He, We,
                                                    K, first_segment, _p(table), _stream()), "seg_contingency")
    return table


# --------------------------------------------------------------------------------------------------
# STEVE epoch visualisation (csrc/slot_vis.hip)
# --------------------------------------------------------------------------------------------------
SLOT_FORM_VIS, SLOT_FORM_RAW = 0, 1           # enum focus_slot_form
VIS_OUT_F32, VIS_OUT_U8 = 0, 1                # enum focus_vis_out


def slot_vis_grid_shape(T, H, W, K, rows):
    """[1,T,3,Hg,Wg] of make_grid(nrow=K+3, padding=2) over `rows` clips."""
    return (1, int(T), 3, int(rows) * (int(H) + 2) + 2, (int(K) + 3) * (int(W) + 2) + 2)


def slot_vis_grid(video, recon, gen, *, attns_vis=None, attn=None, grid=None, rows=8, out_dtype=torch.float32):
    """slot_misc.visualize's video in one launch: per frame the grid of `rows` clips x (video, recon, gen, K slot overlays)
    tiles, 2 pixels of 0.8 between and around them -> [1,T,3,Hg,Wg].  video, recon [B,T,3,H,W] and gen [Bg,T,3,H,W] are fp32
    or bf16, each on its own.  The overlays come from exactly one of
      attns_vis [B,T,K,3,H,W] fp32 (what STEVE.forward / encode return): copied;
      attn [B,T,He*We,K] fp32 or bf16 (the slot update's attention) with grid=(He, We), He | H and We | W: the overlay
        video * a + (1 - a) of the nearest-upsampled mask, in the reference's three fp32 roundings, made on the fly.
    rows is clamped to B, as slicing [:N] does; gen must hold that many clips.  out_dtype float32 gives the reference's
    bits, uint8 what TensorBoard's add_video makes of them ((x * 255).clip(0, 255), truncated; NaN -> 0).  No CPU fallback."""
    if (attns_vis is None) == (attn is None):
        raise ValueError("focus_amd: slot_vis_grid takes exactly one of attns_vis and attn")
    if (attn is None) != (grid is None):
        raise ValueError("focus_amd: slot_vis_grid takes grid=(He, We) with attn, and only with it")
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError("focus_amd: slot_vis_grid writes float32 or uint8 (got %s)" % (out_dtype,))
    if video.dim() != 5 or video.shape[2] != 3 or min(video.shape) < 1:
        raise ValueError("focus_amd: slot_vis_grid takes a non-empty video [B,T,3,H,W]; got %s" % (tuple(video.shape),))
    B, T, _, H, W = (int(s) for s in video.shape)
    if tuple(recon.shape) != tuple(video.shape) or gen.dim() != 5 or tuple(gen.shape[1:]) != tuple(video.shape[1:]) \
            or gen.shape[0] < 1:
        raise ValueError("focus_amd: slot_vis_grid: recon %s and gen %s do not match video %s" % (
            tuple(recon.shape), tuple(gen.shape), tuple(video.shape)))
    rows = min(int(rows), B)
    if rows < 1 or rows > gen.shape[0]:
        raise ValueError("focus_amd: slot_vis_grid: %d rows asked of a gen of %d clips (at least 1)" % (rows, gen.shape[0]))
    slots = attn if attns_vis is None else attns_vis
    if attns_vis is not None:
        if slots.dim() != 6 or tuple(slots.shape[:2]) != (B, T) or tuple(slots.shape[3:]) != (3, H, W) \
                or not 1 <= slots.shape[2] <= 32:
            raise ValueError("focus_amd: slot_vis_grid takes attns_vis [B,T,K,3,H,W] with 1 <= K <= 32; got %s for video %s" % (
                tuple(slots.shape), tuple(video.shape)))
        if slots.dtype != torch.float32:
            raise ValueError("focus_amd: slot_vis_grid: attns_vis is float32 (got %s)" % slots.dtype)
        K, He, We, form = int(slots.shape[2]), 1, 1, SLOT_FORM_VIS
    else:
        try:
            He, We = (int(g) for g in grid)
        except (TypeError, ValueError):
            raise ValueError("focus_amd: slot_vis_grid: grid is (He, We); got %r" % (grid,))
        if He < 1 or We < 1 or H % He or W % We:
            raise ValueError("focus_amd: slot_vis_grid: the %dx%d slot grid does not divide the %dx%d frame" % (He, We, H, W))
        if slots.dim() != 4 or tuple(slots.shape[:3]) != (B, T, He * We) or not 1 <= slots.shape[3] <= 32:
            raise ValueError("focus_amd: slot_vis_grid takes attn [B,T,He*We,K] with 1 <= K <= 32; got %s for video %s and a "
                             "%dx%d grid" % (tuple(slots.shape), tuple(video.shape), He, We))
        K, form = int(slots.shape[3]), SLOT_FORM_RAW
    shape = slot_vis_grid_shape(T, H, W, K, rows)
    if T * 3 * shape[3] * shape[4] >= 2 ** 31:
        raise ValueError("focus_amd: slot_vis_grid: a video of %s has 2^31 elements or more" % (shape,))
    for name, t in (("video", video), ("recon", recon), ("gen", gen), ("attn", slots)):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("focus_amd: slot_vis_grid: %s is float32 or bfloat16 (got %s)" % (name, t.dtype))
        _need_contiguous(t, "slot_vis_grid's %s" % name)
        if t.device != video.device:
            raise ValueError("focus_amd: slot_vis_grid: %s is on %s, video on %s" % (name, t.device, video.device))
    _need_gpu(video)
    out = torch.empty(shape, device=video.device, dtype=out_dtype)
    with torch.cuda.device(video.device):
        _lib.check(_lib.lib().focus_slot_vis_grid(
            _p(video), _dt(video), _p(recon), _dt(recon), _p(gen), _dt(gen), _p(slots), _dt(slots), form, B, int(gen.shape[0]),
            T, 3, H, W, K, He, We, rows, _p(out), VIS_OUT_U8 if out_dtype == torch.uint8 else VIS_OUT_F32, _stream()),
            "slot_vis_grid")
    return out


# --------------------------------------------------------------------------------------------------
# Step and test statistics (csrc/step_stats.hip)
# --------------------------------------------------------------------------------------------------
STATS_INTS, STATS_FLOATS = 16, 8      # the two accumulator tables of focus_topk_stats (include/focus_amd.h)


def _stats_head(h, logits, labels, dense, B):
    if logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16) or logits.stride(1) != 1:
        raise ValueError("focus_amd: topk_stats takes float32 or bfloat16 logits [B,V] with unit column stride; head %d is %s %s "
                         "with strides %s" % (h, logits.dtype, tuple(logits.shape), tuple(logits.stride())))
    if logits.shape[0] != B or labels.device != logits.device:
        raise ValueError("focus_amd: topk_stats: head %d has logits %s on %s and labels %s on %s for a batch of %d" % (
            h, tuple(logits.shape), logits.device, tuple(labels.shape), labels.device, B))
    V = logits.shape[1]
    if dense:
        if labels.dtype != torch.float32 or tuple(labels.shape) != (B, V) or labels.stride(1) != 1 or V < 2:
            raise ValueError("focus_amd: topk_stats: dense labels are float32 [B,V] like the logits, V >= 2; head %d has %s %s "
                             "against logits %s" % (h, labels.dtype, tuple(labels.shape), tuple(logits.shape)))
        ldl = labels.stride(0) if B > 1 else V
    else:
        if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_contiguous():
            raise ValueError("focus_amd: topk_stats: class labels are contiguous int64 [B]; head %d has %s %s for a batch of %d" % (
                h, labels.dtype, tuple(labels.shape), B))
        ldl = 0
    return [_p(logits), _dt(logits), V, logits.stride(0) if B > 1 else V, _p(labels), ldl]


def topk_stats(acc_i, acc_f, preds=(), labels=(), ks=(1, 5), losses=(), batch=None):
    """Adds one batch into the accumulator (acc_i int64 [16], acc_f float64 [8], see include/focus_amd.h): top-k correct counts
    of up to two heads under the order "NaN greatest, ties to the lowest index", the count of rows correct in every head,
    steps, samples, the double sums of up to three 0-d fp32 device losses, and the first step whose losses[0] is NaN.
    preds: a tensor [B,V] or a tuple of one or two (fp32 / bf16; a row stride is passed as it is, nothing is copied);
    labels: per head int64 [B] or dense float32 [B,V] (mixup targets, collapsed inside the kernel).  No heads (STEVE): give
    `batch`.  One launch, no sync, no CPU fallback."""
    preds = (preds,) if isinstance(preds, torch.Tensor) else tuple(preds)
    labels = (labels,) if isinstance(labels, torch.Tensor) else tuple(labels)
    losses = tuple(losses)
    _need_gpu(acc_i, acc_f, *preds, *labels, *losses)
    if acc_i.dtype != torch.int64 or acc_f.dtype != torch.float64 or acc_i.numel() != STATS_INTS or acc_f.numel() != STATS_FLOATS \
            or not acc_i.is_contiguous() or not acc_f.is_contiguous():
        raise ValueError("focus_amd: topk_stats takes accumulators int64 [%d] and float64 [%d]; got %s %s, %s %s" % (
            STATS_INTS, STATS_FLOATS, acc_i.dtype, tuple(acc_i.shape), acc_f.dtype, tuple(acc_f.shape)))
    heads = len(preds)
    if heads > 2 or len(labels) != heads or len(losses) > 3:
        raise ValueError("focus_amd: topk_stats takes at most two heads with one label tensor each and at most three losses; got "
                         "%d heads, %d label tensors, %d losses" % (heads, len(labels), len(losses)))
    for l in losses:
        if l is not None and (l.dtype != torch.float32 or l.numel() != 1):
            raise ValueError("focus_amd: topk_stats takes float32 scalar losses; got %s %s" % (l.dtype, tuple(l.shape)))
    ks = tuple(int(k) for k in ks)
    dense = 0
    if heads:
        B = preds[0].shape[0]
        dense = int(labels[0].is_floating_point())
        if any(int(l.is_floating_point()) != dense for l in labels):
            raise ValueError("focus_amd: topk_stats: the heads' labels are either all class indices or all dense rows")
        head_args = sum((_stats_head(h, p, l, dense, B) for h, (p, l) in enumerate(zip(preds, labels))), [])
        head_args += [None, F32, 0, 0, None, 0] * (2 - heads)
        vmin = min(p.shape[1] for p in preds)
        if not 1 <= len(ks) <= 4 or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])) or ks[-1] > vmin:
            raise ValueError("focus_amd: topk_stats takes 1 to 4 ascending ks between 1 and the smallest class count %d; got %s" % (
                vmin, ks))
    else:
        if batch is None:
            raise ValueError("focus_amd: topk_stats without heads needs the batch size")
        B = int(batch)
        head_args = [None, F32, 0, 0, None, 0] * 2
        ks = ks[:4]
    k4 = list(ks) + [0] * (4 - len(ks))
    l3 = [_p(l) for l in losses] + [None] * (3 - len(losses))
    with torch.cuda.device(acc_i.device):
        _lib.check(_lib.lib().focus_topk_stats(heads, B, *head_args, dense, len(ks), *k4, *l3, _p(acc_i), _p(acc_f), _stream()),
                   "topk_stats")


VIEW_MODES = {"sum": 0, "max": 1}


def view_accumulate(preds, clip_ids, labels, num_clips, video_preds, video_labels, clip_count, flag, mode="sum"):
    """Multi-view ensembling of one head: row i of preds [n,C] (fp32 / bf16, a row stride is passed as it is) is folded into
    row clip_ids[i] // num_clips of video_preds fp32 [num_videos,C], rows of one video in ascending row order; video_labels
    and clip_count (int64 [num_videos]) follow; flag int32 [1] gets bit 0 for a clip contradicting its video's label and
    bit 1 for a clip id out of range.  One launch, no sync, no CPU fallback."""
    _need_gpu(preds, clip_ids, labels, video_preds, video_labels, clip_count, flag)
    if mode not in VIEW_MODES:
        raise ValueError("focus_amd: view_accumulate's mode is 'sum' or 'max'; got %r" % (mode,))
    if preds.dim() != 2 or preds.dtype not in (torch.float32, torch.bfloat16) or preds.stride(1) != 1:
        raise ValueError("focus_amd: view_accumulate takes float32 or bfloat16 preds [n,C] with unit column stride; got %s %s with "
                         "strides %s" % (preds.dtype, tuple(preds.shape), tuple(preds.stride())))
    n, C = preds.shape
    for t, what in ((clip_ids, "clip_ids"), (labels, "labels")):
        if t.dtype != torch.int64 or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError("focus_amd: view_accumulate takes contiguous int64 %s [%d]; got %s %s" % (what, n, t.dtype, tuple(t.shape)))
    if video_preds.dim() != 2 or video_preds.shape[1] != C or video_preds.dtype != torch.float32 or not video_preds.is_contiguous():
        raise ValueError("focus_amd: view_accumulate takes a contiguous float32 table [num_videos,%d]; got %s %s" % (
            C, video_preds.dtype, tuple(video_preds.shape)))
    NV = video_preds.shape[0]
    for t, what in ((video_labels, "video_labels"), (clip_count, "clip_count")):
        if t.dtype != torch.int64 or tuple(t.shape) != (NV,) or not t.is_contiguous():
            raise ValueError("focus_amd: view_accumulate takes contiguous int64 %s [%d]; got %s %s" % (what, NV, t.dtype, tuple(t.shape)))
    if flag.dtype != torch.int32 or flag.numel() != 1 or int(num_clips) < 1 or C < 1:
        raise ValueError("focus_amd: view_accumulate takes an int32 flag of one element, num_clips >= 1 and C >= 1; got %s %s, %s, %d"
                         % (flag.dtype, tuple(flag.shape), num_clips, C))
    with torch.cuda.device(preds.device):
        _lib.check(_lib.lib().focus_view_accumulate(_p(preds), _dt(preds), n, C, preds.stride(0) if n > 1 else C, _p(clip_ids),
                                                    _p(labels), int(num_clips), NV, VIEW_MODES[mode], _p(video_preds),
                                                    _p(video_labels), _p(clip_count), _p(flag), _stream()), "view_accumulate")


# --------------------------------------------------------------------------------------------------
# The multi-label route (csrc/multilabel.hip): BCE losses, the dense view table, average precision
# --------------------------------------------------------------------------------------------------
BCE_MODES = {"logits": 0, "probs": 1}                                      # enum focus_bce_mode


class _BceRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mode, mean):
        R, C = x.shape
        xf = x.float()
        if xf.stride(1) != 1:
            xf = xf.contiguous()
        loss_rows = torch.empty(R, device=x.device, dtype=torch.float32)
        dx = torch.empty((R, C), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().focus_bce_rows(_p(xf), xf.stride(0) if R > 1 else C, _p(y), y.stride(0) if R > 1 else C, R, C,
                                                 BCE_MODES[mode], 1.0 / (R * C) if mean else 1.0, _p(loss_rows), _p(dx), C,
                                                 _stream()), "bce_rows")
        ctx.save_for_backward(dx)
        ctx.dtype = x.dtype
        total = loss_rows.sum()                                 # R values; the rows themselves were summed in a fixed order
        return total / (R * C) if mean else total

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors                   # d(mean or sum) / dx
        return (dx * g.float()).to(ctx.dtype), None, None, None


def _bce(x, y, reduction, mode, what):
    _need_gpu(x, y)
    if reduction not in ("mean", "sum"):
        raise NotImplementedError("focus_amd: %s reduction is 'mean' or 'sum' (got %r); the train loops use no other" % (
            what, reduction))
    if x.dim() != 2 or x.shape != y.shape or x.numel() == 0 or y.device != x.device:
        raise ValueError("focus_amd: %s takes inputs and targets of one [R,C] shape on one device (got %s on %s and %s on %s)" % (
            what, tuple(x.shape), x.device, tuple(y.shape), y.device))
    _dt(x)
    y = y.detach().float()
    if y.stride(1) != 1:
        y = y.contiguous()
    return _BceRowsFn.apply(x, y, mode, reduction == "mean")


def bce_with_logits(x, y, reduction="mean"):
    """nn.BCEWithLogitsLoss: max(x,0) - x y + log1p(exp(-|x|)) summed or averaged over all elements, value and gradient
    (sigmoid(x) - y) from one row kernel.  x [R,C] fp32 or bf16 (widened first; the gradient comes back in x's type), y
    [R,C] targets in [0,1] (used as fp32; no gradient flows into them).  A row stride is passed as it is."""
    return _bce(x, y, reduction, "logits", "bce_with_logits")


def bce(p, y, reduction="mean"):
    """nn.BCELoss on probabilities p [R,C] in [0,1], with ATen's clamps: the logs at -100, the gradient's denominator at
    1e-12.  Values outside [0,1], for which torch raises, give NaN: a check would cost a sync."""
    return _bce(p, y, reduction, "probs", "bce")


def view_accumulate_dense(preds, clip_ids, labels, num_clips, video_preds, video_labels, clip_count, flag, mode="sum"):
    """view_accumulate for multi-label videos: labels are dense float32 rows [n,C] (a row stride is passed as it is),
    video_labels is float32 [num_videos,C].  flag bit 0: the row stored for a video had a positive entry and a clip of that
    video came with another row; bit 1: a clip id out of range.  One launch, no sync, no CPU fallback."""
    _need_gpu(preds, clip_ids, labels, video_preds, video_labels, clip_count, flag)
    if mode not in VIEW_MODES:
        raise ValueError("focus_amd: view_accumulate_dense's mode is 'sum' or 'max'; got %r" % (mode,))
    if preds.dim() != 2 or preds.dtype not in (torch.float32, torch.bfloat16) or preds.stride(1) != 1:
        raise ValueError("focus_amd: view_accumulate_dense takes float32 or bfloat16 preds [n,C] with unit column stride; got %s %s "
                         "with strides %s" % (preds.dtype, tuple(preds.shape), tuple(preds.stride())))
    n, C = preds.shape
    if clip_ids.dtype != torch.int64 or tuple(clip_ids.shape) != (n,) or not clip_ids.is_contiguous():
        raise ValueError("focus_amd: view_accumulate_dense takes contiguous int64 clip_ids [%d]; got %s %s" % (
            n, clip_ids.dtype, tuple(clip_ids.shape)))
    if labels.dtype != torch.float32 or tuple(labels.shape) != (n, C) or labels.stride(1) != 1:
        raise ValueError("focus_amd: view_accumulate_dense takes float32 labels [%d,%d] with unit column stride; got %s %s with "
                         "strides %s" % (n, C, labels.dtype, tuple(labels.shape), tuple(labels.stride())))
    for t, what in ((video_preds, "video_preds"), (video_labels, "video_labels")):
        if t.dim() != 2 or t.shape[1] != C or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("focus_amd: view_accumulate_dense takes a contiguous float32 %s [num_videos,%d]; got %s %s" % (
                what, C, t.dtype, tuple(t.shape)))
    NV = video_preds.shape[0]
    if video_labels.shape[0] != NV or clip_count.dtype != torch.int64 or tuple(clip_count.shape) != (NV,) \
            or not clip_count.is_contiguous():
        raise ValueError("focus_amd: view_accumulate_dense takes video_labels [%d,%d] and contiguous int64 clip_count [%d]; got %s "
                         "and %s %s" % (NV, C, NV, tuple(video_labels.shape), clip_count.dtype, tuple(clip_count.shape)))
    if flag.dtype != torch.int32 or flag.numel() != 1 or int(num_clips) < 1 or C < 1:
        raise ValueError("focus_amd: view_accumulate_dense takes an int32 flag of one element, num_clips >= 1 and C >= 1; got %s "
                         "%s, %s, %d" % (flag.dtype, tuple(flag.shape), num_clips, C))
    with torch.cuda.device(preds.device):
        _lib.check(_lib.lib().focus_view_accumulate_dense(
            _p(preds), _dt(preds), n, C, preds.stride(0) if n > 1 else C, _p(clip_ids), _p(labels), labels.stride(0) if n > 1 else C,
            int(num_clips), NV, VIEW_MODES[mode], _p(video_preds), _p(video_labels), _p(clip_count), _p(flag), _stream()),
            "view_accumulate_dense")


AP_BAD_LABEL, AP_BAD_SCORE, AP_NO_CLASS = 1, 2, 4                          # the bits of focus_average_precision's flag


def average_precision(scores, labels):
    """scikit-learn's average_precision_score(labels, scores, average=None) over the columns of a device table, by counting
    (include/focus_amd.h): scores and labels float32 [N,C], labels 0 or 1, row strides passed as they are.  Returns
    (ap float64 [C], npos int64 [C], summary float64 [2] = (mean ap over the classes with a positive, their number), flag
    int32 [1]: AP_BAD_LABEL | AP_BAD_SCORE | AP_NO_CLASS).  Classes without a positive have ap 0 and are left out of the
    mean.  Nothing is synchronised and nothing is read back here; no CPU fallback."""
    _need_gpu(scores, labels)
    if scores.dim() != 2 or scores.shape != labels.shape or scores.dtype != torch.float32 or labels.dtype != torch.float32 \
            or scores.stride(1) != 1 or labels.stride(1) != 1 or scores.shape[1] < 1 or labels.device != scores.device:
        raise ValueError("focus_amd: average_precision takes float32 scores and labels of one [N,C] shape, C >= 1, with unit column "
                         "stride on one device; got %s %s %s on %s and %s %s %s on %s" % (
                             scores.dtype, tuple(scores.shape), tuple(scores.stride()), scores.device, labels.dtype,
                             tuple(labels.shape), tuple(labels.stride()), labels.device))
    N, C = scores.shape
    dev = scores.device
    ap = torch.zeros(C, dtype=torch.float64, device=dev)
    npos = torch.zeros(C, dtype=torch.int64, device=dev)
    summary = torch.zeros(2, dtype=torch.float64, device=dev)
    flag = torch.full((1,), AP_NO_CLASS, dtype=torch.int32, device=dev)     # what an empty table is left with
    if N == 0:
        return ap, npos, summary, flag
    L = _lib.lib()
    nbytes = L.focus_average_precision_workspace_bytes(N, C)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.focus_average_precision(_p(scores), scores.stride(0) if N > 1 else C, _p(labels),
                                             labels.stride(0) if N > 1 else C, N, C, _p(npos), _p(ap), _p(summary), _p(flag),
                                             _p(ws), nbytes, _stream()), "average_precision")
    return ap, npos, summary, flag


# --------------------------------------------------------------------------------------------------
# the AVA evaluation (csrc/ava_eval.hip)
# --------------------------------------------------------------------------------------------------
AVA_GT_OVERFLOW, AVA_BAD_INDEX = 1, 2                                      # the bits of focus_ava_match's flag
VOC_BAD_SCORE, VOC_TP_ABOVE_GT, VOC_GT_ABOVE_TOTAL = 1, 2, 4               # the bits of focus_voc_ap's flag
AVA_GT_CAP = 64                                                            # ground-truth rows per (image, class)


def _need_table(t, dtype, shape, what, fn):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("focus_amd: %s takes a contiguous %s %s %s; got %s %s" % (
            fn, str(dtype).replace("torch.", ""), what, list(shape), t.dtype, tuple(t.shape)))


def ava_match(boxes, num_classes, grp_off, det_rows, grp_image, gt_off, gt_class, gt_boxes, whitelist, out=None, counts=None,
              flag=None):
    """The greedy match of the AVA evaluation per (image, class) (include/focus_amd.h): boxes float32 [K,4] (x1, y1, x2, y2) in
    arrival order; grp_off int64 [G+1], det_rows int64 [K], grp_image int64 [G] group the rows by image; gt_off int64 [I+1],
    gt_class int32 [R], gt_boxes float64 [R,4] are the ground truth by image; whitelist uint8 [C].  Returns (bytes uint8 [K,C]:
    0 not evaluated, 1 false positive, 2 true positive; counts int64 [2,C]: judged rows and true positives per class, added
    to; flag int32 [1]: AVA_GT_OVERFLOW | AVA_BAD_INDEX, sticky).  One launch, no sync, no CPU fallback."""
    _need_gpu(boxes, grp_off, det_rows, grp_image, gt_off, gt_class, gt_boxes, whitelist, out, counts, flag)
    fn = "ava_match"
    C = int(num_classes)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or C < 1:
        raise ValueError("focus_amd: ava_match takes boxes [K,4] and num_classes >= 1; got %s, %d" % (tuple(boxes.shape), C))
    K, G, I, R = boxes.shape[0], grp_image.shape[0], gt_off.shape[0] - 1, gt_class.shape[0]
    dev = boxes.device
    _need_table(boxes, torch.float32, (K, 4), "boxes", fn)
    _need_table(grp_off, torch.int64, (G + 1,), "grp_off", fn)
    _need_table(det_rows, torch.int64, (K,), "det_rows", fn)
    _need_table(grp_image, torch.int64, (G,), "grp_image", fn)
    _need_table(gt_off, torch.int64, (I + 1,), "gt_off", fn)
    _need_table(gt_class, torch.int32, (R,), "gt_class", fn)
    _need_table(gt_boxes, torch.float64, (R, 4), "gt_boxes", fn)
    _need_table(whitelist, torch.uint8, (C,), "whitelist", fn)
    if out is None:
        out = torch.zeros((K, C), dtype=torch.uint8, device=dev)
    if counts is None:
        counts = torch.zeros((2, C), dtype=torch.int64, device=dev)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _need_table(out, torch.uint8, (K, C), "out", fn)
    _need_table(counts, torch.int64, (2, C), "counts", fn)
    _need_table(flag, torch.int32, (1,), "flag", fn)
    if any(t.device != dev for t in (grp_off, det_rows, grp_image, gt_off, gt_class, gt_boxes, whitelist, out, counts, flag)):
        raise ValueError("focus_amd: ava_match takes all its tables on one device")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().focus_ava_match(_p(boxes), K, C, _p(grp_off), _p(det_rows), _p(grp_image), G, _p(gt_off),
                                              _p(gt_class), _p(gt_boxes), I, _p(whitelist), _p(out), C, _p(counts), _p(flag),
                                              _stream()), fn)
    return out, counts, flag


def voc_average_precision(scores, bytes_, n_gt, total_gt):
    """The VOC average precision per class from ava_match's byte table (include/focus_amd.h): scores float32 or bfloat16 [N,C]
    (a row stride is passed as it is), bytes_ uint8 [N,C], n_gt int64 [C] the ground-truth rows per class, total_gt a host
    integer >= their sum.  Equal scores are ordered by descending row index.  Returns (ap float64 [C], NaN without ground
    truth; summary float64 [2] = (mean over the classes with ground truth, their number); flag int32 [1]: VOC_BAD_SCORE |
    VOC_TP_ABOVE_GT | VOC_GT_ABOVE_TOTAL).  Nothing is synchronised and nothing is read back here; no CPU fallback."""
    _need_gpu(scores, bytes_, n_gt)
    if scores.dim() != 2 or scores.dtype not in (torch.float32, torch.bfloat16) or scores.shape[1] < 1 or \
            (scores.shape[0] > 0 and scores.stride(1) != 1):
        raise ValueError("focus_amd: voc_average_precision takes float32 or bfloat16 scores [N,C], C >= 1, with unit column "
                         "stride; got %s %s with strides %s" % (scores.dtype, tuple(scores.shape), tuple(scores.stride())))
    N, C = scores.shape
    dev = scores.device
    _need_table(bytes_, torch.uint8, (N, C), "bytes", "voc_average_precision")
    _need_table(n_gt, torch.int64, (C,), "n_gt", "voc_average_precision")
    total_gt = int(total_gt)
    if total_gt < 0 or bytes_.device != dev or n_gt.device != dev:
        raise ValueError("focus_amd: voc_average_precision takes total_gt >= 0 and all its tables on one device")
    ap = torch.zeros(C, dtype=torch.float64, device=dev)
    summary = torch.zeros(2, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = L.focus_voc_ap_workspace_bytes(N, C, total_gt)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.focus_voc_ap(_p(scores), _dt(scores), scores.stride(0) if N > 1 else C, _p(bytes_), C, N, C, _p(n_gt),
                                  total_gt, _p(ap), _p(summary), _p(flag), _p(ws), nbytes, _stream()), "voc_ap")
    return ap, summary, flag


# --------------------------------------------------------------------------------------------------
# Pooling attention in token layout (csrc/token_pool.hip): the attention_pool of MViT without its permutes
# --------------------------------------------------------------------------------------------------
_POOL_MODES = {"conv": _lib.POOL_CONV, "max": _lib.POOL_MAX, "avg": _lib.POOL_AVG}


def _triple(v):
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(a) for a in v)
    if len(v) != 3:
        raise ValueError("focus_amd: a pooling window takes 3 extents (t, h, w), got %s" % (v,))
    return v


def _norm_parts(norm):
    """None, an nn.LayerNorm-like module or (gamma, beta, eps) -> (gamma, beta, eps) or (None, None, 0.0)."""
    if norm is None:
        return None, None, 0.0
    if isinstance(norm, (tuple, list)):
        return norm[0], norm[1], float(norm[2])
    return norm.weight, norm.bias, float(norm.eps)


def token_pool_ok(x, head_dim, mode, kernel, stride, padding, norm, weight=None):
    """True when ops.token_pool takes this call: x a device [B, N, C] fp32 / bf16 row view with unit column stride and
    16-byte aligned rows, head_dim % 8 == 0 dividing C <= 4096 (<= 128 in conv mode or with a norm), windows 1..7, strides
    1..8, padding below the window (a max window of at most 127 taps), fp32 dense norm parameters and conv weight."""
    if not (torch.is_tensor(x) and x.is_cuda):
        return False
    gamma, beta, _ = _norm_parts(norm)
    if any(t is not None and not t.is_cuda for t in (gamma, beta, weight)):
        return False
    return _token_pool_limits_ok(x, head_dim, mode, kernel, stride, padding, norm, weight)


def _token_pool_limits_ok(x, head_dim, mode, kernel, stride, padding, norm, weight=None):
    """token_pool_ok without its device test: shapes, types, strides and the kernels' limits."""
    if not (x.dim() == 3 and x.dtype in (torch.float32, torch.bfloat16)):
        return False
    if mode not in _POOL_MODES:
        return False
    try:
        k, s, p = _triple(kernel), _triple(stride), _triple(padding)
    except (TypeError, ValueError):
        return False
    B, N, C = x.shape
    head_dim = int(head_dim)
    if head_dim < 8 or head_dim % 8 or C % head_dim or C > 4096 or x.numel() >= 2 ** 31:
        return False
    gamma, beta, _ = _norm_parts(norm)
    if (mode == "conv" or gamma is not None) and head_dim > 128:
        return False
    if any(not 1 <= a <= 7 for a in k) or any(not 1 <= a <= 8 for a in s) or any(not 0 <= a < b for a, b in zip(p, k)):
        return False
    if mode == "max" and k[0] * k[1] * k[2] > 127:
        return False
    a = 16 // x.element_size()
    if B > 0 and N > 0 and (x.stride(2) != 1 or x.stride(1) < C or x.stride(1) % a or x.stride(0) % a or x.data_ptr() % 16):
        return False
    for t in (gamma, beta, weight):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous()):
            return False
    if (gamma is None) != (beta is None) or (gamma is not None and (gamma.numel() != head_dim or beta.numel() != head_dim)):
        return False
    if mode == "conv" and weight is not None and weight.numel() != head_dim * k[0] * k[1] * k[2]:
        return False
    return True


def _pool_desc(x, shape, thw, mode, k, s, p, cls, head_dim, dt):
    """The descriptor of a call; x (None: dense) gives the strides of the input view."""
    B, N, C = shape
    d = _lib.TokenPoolDesc()
    d.B, d.T, d.H, d.W, d.C, d.head_dim, d.cls = B, thw[0], thw[1], thw[2], C, head_dim, cls
    for i in range(3):
        d.k[i], d.s[i], d.p[i] = k[i], s[i], p[i]
    d.mode, d.dtype = mode, dt
    d.x_batch_stride, d.x_row_stride = (x.stride(0), x.stride(1)) if x is not None and B > 0 and N > 0 else (N * C, C)
    return d


class _TokenPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, cfg):
        thw, thw_out, mode, k, s, p, cls, head_dim, eps, keep = cfg
        B, N, C = x.shape
        rows_out = cls + thw_out[0] * thw_out[1] * thw_out[2]
        heads = C // head_dim
        dev = x.device
        d = _pool_desc(x, x.shape, thw, mode, k, s, p, cls, head_dim, _dt(x))
        y = torch.empty(B, rows_out, C, device=dev, dtype=x.dtype)
        norm = gamma is not None
        pooled = mean = rstd = idx = None
        if norm and keep:
            pooled = torch.empty_like(y)
            mean = torch.empty(B * rows_out * heads, device=dev, dtype=torch.float32)
            rstd = torch.empty_like(mean)
        if mode == _lib.POOL_MAX:
            idx = torch.empty(B, rows_out, C, device=dev, dtype=torch.int8)
        _lib.check(_lib.lib().focus_token_pool_fwd(ctypes.byref(d), _p(x), _p(weight), _p(gamma), _p(beta), eps, _p(y), _p(pooled),
                                                   _p(mean), _p(rstd), _p(idx), _stream()), "token_pool_fwd")
        if keep:
            ctx.save_for_backward(x if (mode == _lib.POOL_CONV and ctx.needs_input_grad[1]) else None, weight, idx,
                                  pooled, mean, rstd, gamma)
            ctx.cfg = cfg
            ctx.x_meta = (tuple(x.shape), x.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, idx, pooled, mean, rstd, gamma = ctx.saved_tensors
        thw, thw_out, mode, k, s, p, cls, head_dim, eps, _ = ctx.cfg
        (B, N, C), dtype = ctx.x_meta
        L = _lib.lib()
        dev = dy.device
        if dy.dtype != dtype:
            dy = dy.to(dtype)
        if not dy.is_contiguous():
            dy = dy.contiguous()
        dg = db = None
        dp = dy
        if gamma is not None:
            # the per-head LayerNorm backward: the existing kernel on the [B*rows*heads, head_dim] view of the pooled rows
            rows = mean.shape[0]
            dp = torch.empty_like(pooled)
            dg = torch.empty(head_dim, device=dev, dtype=torch.float32)
            db = torch.empty(head_dim, device=dev, dtype=torch.float32)
            partial = torch.empty(2, L.focus_layernorm_bwd_blocks(rows), head_dim, device=dev, dtype=torch.float32)
            _lib.check(L.focus_layernorm_bwd(_p(dy), _p(pooled), _p(gamma), _p(mean), _p(rstd), None, _p(dp), _p(dg), _p(db),
                                             _p(partial), rows, head_dim, _dt(pooled), _stream()), "layernorm_bwd")
        want_dx = ctx.needs_input_grad[0]
        want_dw = mode == _lib.POOL_CONV and ctx.needs_input_grad[1]
        dx = dw = ws = None
        nbytes = 0
        if want_dx:
            dx = torch.empty(B, N, C, device=dev, dtype=dtype)
        if want_dx or want_dw:
            d = _pool_desc(x if want_dw else None, (B, N, C), thw, mode, k, s, p, cls, head_dim, _dt(dp))
            if want_dw:
                dw = torch.empty(weight.shape, device=dev, dtype=torch.float32)
                nbytes = L.focus_token_pool_workspace_bytes(ctypes.byref(d))
                ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
            _lib.check(L.focus_token_pool_bwd(ctypes.byref(d), _p(dp), _p(x) if want_dw else None, _p(weight), _p(idx), _p(dx),
                                              _p(dw), _p(ws), nbytes, _stream()), "token_pool_bwd")
        return dx, dw, dg, db, None


def token_pool(x, thw, mode, weight, kernel, stride, padding, has_cls, head_dim, norm=None):
    """attention_pool in token layout on the HIP kernels: x [B, cls + T*H*W, C] rows (heads = column blocks of head_dim; a
    strided row view is read in place) -> (y [B, cls + T'*H'*W', C], [T', H', W']).  mode 'conv' (weight: the depth-wise
    Conv3d.weight [head_dim, 1, kt, kh, kw], fp32, no bias), 'max' or 'avg' (count_include_pad).  norm: None, an nn.LayerNorm
    over head_dim or (gamma, beta, eps): fused per head, from the un-rounded fp32 pooled values, the cls row included.
    Gradients go to x, weight, gamma and beta; under torch.no_grad() nothing is kept.  No CPU fallback."""
    gamma, beta, eps = _norm_parts(norm)
    _need_gpu(x, weight, gamma, beta)
    if mode not in _POOL_MODES:
        raise ValueError("focus_amd: token_pool mode is 'conv', 'max' or 'avg' (got %r)" % (mode,))
    k, s, p = _triple(kernel), _triple(stride), _triple(padding)
    thw = [int(a) for a in thw]
    cls = 1 if has_cls else 0
    if x.dim() != 3 or x.shape[1] != cls + thw[0] * thw[1] * thw[2]:
        raise RuntimeError("focus_amd: token_pool takes [B, %d + T*H*W, C] rows for the grid %s (got %s)" % (cls, thw, tuple(x.shape)))
    if mode == "conv":
        if weight is None or weight.dtype != torch.float32 or not weight.is_contiguous() or \
                weight.numel() != int(head_dim) * k[0] * k[1] * k[2]:
            raise RuntimeError("focus_amd: token_pool in conv mode takes a dense fp32 weight [head_dim, 1, kt, kh, kw]")
    else:
        weight = None
    for t in (gamma, beta):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != int(head_dim)):
            raise RuntimeError("focus_amd: token_pool's norm parameters are dense fp32 vectors of head_dim")
    if x.shape[0] > 0 and x.stride(2) != 1:
        x = x.contiguous()
    thw_out = [(thw[i] + 2 * p[i] - k[i]) // s[i] + 1 for i in range(3)]
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, gamma, beta))
    cfg = (tuple(thw), tuple(thw_out), _POOL_MODES[mode], k, s, p, cls, int(head_dim), eps, keep)
    return _TokenPoolFn.apply(x, weight, gamma, beta, cfg), thw_out
