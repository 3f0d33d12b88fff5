"""Plain fp64 formulas of the slot-attention step (csrc/slot_attn.hip; steve.py:76-83) and the case table of
tests/test_gpu_slot_attn.py.  Checked without a GPU by tests/test_slot_attn_ref_cpu.py (the closed-form backward against
torch.autograd, every case's route against focus_slot_attn_route); the product never imports this, and this imports
neither a GPU nor focus_amd.

  forward(k, v, q, eps)          attn_vis = softmax_k(k q^T), colsum[b,k] = sum_n (attn + eps), updates = ((attn+eps)/colsum)^T v
  backward(k, v, q, attn, colsum, upd, dupd, dattn | None, eps)
                                 the closed form the kernels use, as a function of the SAVED forward tensors:
                                     r[k] = dupd[k] . upd[k]            dav = (dupd . v - r) / colsum (+ dattn)
                                     dl = a (dav - sum_k a dav)         w = (a + eps) / colsum
                                     dk = dl q      dv = w dupd      dq = dl^T k
                                 and the magnitudes Check.tight(..., mag=) expects (the scale of the rounding error of a sum
                                 that cancels): dlg = a (|dav| + sum_k a |dav|), mag_k = dlg |q|, mag_q = dlg^T |k|,
                                 mag_v = w |dupd|; mag_k_terms, mag_q_terms: the same from the terms of dav (fp32 routes)
  kv_grad(wls, qs, dupds)        dk = sum_i dlogits_i q_i, dv = sum_i w_i dupd_i from stored (w | dlogits) rows [B,N,32]
  inputs(case)                   seeded inputs, rounded to the case's dtype
Nothing is rounded in here: every function takes the values a kernel READS (any float tensor) and returns fp64."""
import collections

import torch

# focus_slot_kernel of include/focus_amd.h
FWD_MFMA, FWD_GENERIC, BWD_DEFER, BWD_MFMA, BWD_GENERIC = 1, 2, 3, 4, 5
KERNEL_NAMES = {FWD_MFMA: "slot_fwd_mfma_kernel", FWD_GENERIC: "slot_fwd_kernel", BWD_DEFER: "slot_bwd_defer_kernel",
                BWD_MFMA: "slot_bwd_mfma_kernel", BWD_GENERIC: "slot_bwd_kernel"}


def decode_route(code):
    """focus_slot_attn_route's value -> (kernel, full, p0, p1); a negative status is returned as it is."""
    if code < 0:
        return code
    return code & 0xFF, (code >> 8) & 1, (code >> 16) & 0xFF, (code >> 24) & 0xFF


# ---- the formulas ---------------------------------------------------------------------------------------------------
def forward(k, v, q, eps):
    """k, v [B,N,D], q [B,K,D] -> attn_vis [B,N,K], colsum [B,K], updates [B,K,D]."""
    k, v, q = k.double(), v.double(), q.double()
    attn = torch.softmax(k @ q.transpose(-1, -2), dim=-1)
    aa = attn + eps
    colsum = aa.sum(dim=-2)
    upd = (aa / colsum.unsqueeze(-2)).transpose(-1, -2) @ v
    return attn, colsum, upd


def backward(k, v, q, attn, colsum, upd, dupd, dattn, eps):
    """-> dict(w, dlogits, dk, dv, dq, dlg, mag_k, mag_v, mag_q), all fp64, from the saved attn [B,N,K], colsum [B,K] and
    upd [B,K,D], the cotangents dupd [B,K,D] and dattn [B,N,K] (or None)."""
    k, v, q, attn, colsum, upd, dupd = (t.double() for t in (k, v, q, attn, colsum, upd, dupd))
    cs = colsum.unsqueeze(-2)                                         # [B,1,K]
    r = (dupd * upd).sum(-1).unsqueeze(-2)                            # [B,1,K]
    dav = (v @ dupd.transpose(-1, -2) - r) / cs
    if dattn is not None:
        dav = dav + dattn.double()
    dl = attn * (dav - (attn * dav).sum(-1, keepdim=True))
    w = (attn + eps) / cs
    dlg = attn * (dav.abs() + (attn * dav.abs()).sum(-1, keepdim=True))
    # the same with the TERMS of dav in place of dav: dupd . v - r is itself a difference (with one input row it is 0 but
    # for the rounding of the stored updates), so an fp32 kernel's error in it scales with sum_d |dupd v| + sum_d |dupd upd|,
    # not with |dav|.  The fp32 routes are held to these (their whole error is fp32 accumulation, a fraction of the terms);
    # the bf16 routes to dlg (their error is the rounding of stored values and operands, a fraction of the values).
    gterms = (v.abs() @ dupd.abs().transpose(-1, -2) + (dupd * upd).abs().sum(-1).unsqueeze(-2)) / cs
    if dattn is not None:
        gterms = gterms + dattn.double().abs()
    dlt = attn * (gterms + (attn * gterms).sum(-1, keepdim=True))
    return {"w": w, "dlogits": dl, "dk": dl @ q, "dv": w @ dupd, "dq": dl.transpose(-1, -2) @ k, "dlg": dlg,
            "mag_k": dlg @ q.abs(), "mag_v": w @ dupd.abs(), "mag_q": dlg.transpose(-1, -2) @ k.abs(),
            "mag_k_terms": dlt @ q.abs(), "mag_q_terms": dlt.transpose(-1, -2) @ k.abs()}


def kv_grad(wls, qs, dupds):
    """wls: (w | dlogits) rows [B,N,32] per iteration (slots 0..15 | 16..31), qs / dupds [B,K,D] -> dk, dv, mag_k, mag_v."""
    dk = dv = mk = mv = 0.0
    for wl, q, du in zip(wls, qs, dupds):
        K = q.shape[1]
        w, dl = wl.double()[..., :K], wl.double()[..., 16:16 + K]
        dk, dv = dk + dl @ q.double(), dv + w @ du.double()
        mk, mv = mk + dl.abs() @ q.double().abs(), mv + w.abs() @ du.double().abs()
    return dk, dv, mk, mv


# ---- the cases ------------------------------------------------------------------------------------------------------
# fwd / bwd: the route the case is meant to reach, (kernel, FULL, KS or KP, DV or 0).  wl: the deferred backward (the
# launch writes (w | dlogits) rows, focus_slot_kv_grad forms dk, dv); else the backward writes dk, dv itself and a second
# call adds to them (accumulate = 1).  da: whether the first / second backward call gets a cotangent of attn_vis (else NULL).
# kv_gap / attn_gap: elements between two batch elements; k_off: elements k_t starts behind a 16-byte boundary.
# big: k scaled so that the logits span about +-20 (the max-subtraction works).  hand: FOCUS_SLOT_HAND for the calls.
Case = collections.namedtuple("Case", "name dtype B N K D eps big wl da kv_gap attn_gap k_off hand fwd bwd")
EPS_SMALL, EPS_BIG = 1e-8, 0.05


def _mf(D, full):
    return (FWD_MFMA, full, D // 32, 0)


def _gen(kernel, K, D):
    return (kernel, 0, 4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32, (D + 63) // 64)


def _case(name, dtype, B, N, K, D, route, eps=EPS_SMALL, big=False, wl=False, da=(True, False), kv_gap=0, attn_gap=0,
          k_off=0, hand=None):
    if route == "generic":
        fwd, bwd = _gen(FWD_GENERIC, K, D), _gen(BWD_GENERIC, K, D)
    else:
        full = int(route == "full")
        fwd = _mf(D, full)
        bwd = (BWD_DEFER, full, D // 32, 0) if wl else (BWD_MFMA, 0, D // 32, 0)
    return Case(name, dtype, B, N, K, D, eps, big, wl, da, kv_gap, attn_gap, k_off, hand, fwd, bwd)


def _build():
    c = []
    # forward MFMA FULL + deferred backward FULL, hand-issued loads; each backward instantiation with and without dattn
    for i, (B, N, K, D) in enumerate([(2, 256, 11, 192), (1, 512, 16, 64), (2, 256, 5, 128), (1, 256, 16, 256)]):
        c.append(_case("full_k%d_d%d" % (K, D), "bf16", B, N, K, D, "full", wl=True, eps=EPS_BIG if i in (1, 2) else EPS_SMALL,
                       big=i % 2 == 1, da=(True, False) if i % 2 == 0 else (False, True)))
    c.append(_case("nohand_k11_d192", "bf16", 2, 256, 11, 192, "ragged", wl=True, hand="0"))
    # ragged last workgroup, deferred backward
    # (N = 1 with dattn on both calls: with one row updates = v, so dupd . v - r is 0 and without dattn the whole gradient
    # of the logits is the rounding residue of the stored updates -- nothing a bound relative to |d attn| can judge)
    for i, N in enumerate([1, 15, 16, 17, 33, 255, 257, 700]):
        c.append(_case("ragged_n%d" % N, "bf16", 2, N, 11, 192, "ragged", wl=True, big=i % 2 == 1,
                       eps=EPS_BIG if N in (17, 255) else EPS_SMALL,
                       da=(True, True) if N == 1 else (True, False) if i % 2 == 0 else (False, True)))
    c.append(_case("ragged_k1", "bf16", 3, 300, 1, 64, "ragged", wl=True))
    c.append(_case("ragged_k16_d256", "bf16", 2, 77, 16, 256, "ragged", wl=True, big=True, da=(False, True)))
    c.append(_case("ragged_k7_d128", "bf16", 2, 1000, 7, 128, "ragged", wl=True, eps=EPS_BIG))
    # slot_bwd_mfma_kernel (no wl): accumulate 0 then 1
    for D in (64, 128, 192, 256):
        for N in (256, 257, 33):
            for K in (3, 16):
                i = len(c)
                c.append(_case("direct_n%d_k%d_d%d" % (N, K, D), "bf16", 2, N, K, D, "full" if N == 256 else "ragged",
                               big=i % 2 == 1, eps=EPS_BIG if i % 3 == 0 else EPS_SMALL,
                               da=(True, False) if i % 4 < 2 else (False, True)))
    # batch strides
    c.append(_case("gaps_defer", "bf16", 3, 257, 11, 192, "ragged", wl=True, kv_gap=64, attn_gap=24))
    c.append(_case("gaps_direct", "bf16", 3, 257, 11, 192, "ragged", kv_gap=64, attn_gap=24, big=True))
    c.append(_case("gap4_generic", "bf16", 3, 257, 11, 192, "generic", kv_gap=4, attn_gap=24))
    c.append(_case("misaligned_k", "bf16", 2, 257, 11, 192, "generic", k_off=1, da=(False, True)))
    # generic kernels
    for i, (B, N, K, D) in enumerate([(2, 130, 3, 64), (2, 65, 8, 100), (1, 64, 11, 192), (2, 129, 16, 256), (2, 100, 17, 40),
                                      (1, 63, 32, 256), (2, 1, 4, 8)]):
        c.append(_case("f32_n%d_k%d_d%d" % (N, K, D), "f32", B, N, K, D, "generic", big=i % 2 == 1,
                       eps=EPS_BIG if i in (1, 4) else EPS_SMALL, da=(True, False) if i % 2 == 0 else (False, True)))
    c.append(_case("bf16_k20_d192", "bf16", 2, 130, 20, 192, "generic"))
    c.append(_case("bf16_k7_d96", "bf16", 2, 65, 7, 96, "generic", big=True, eps=EPS_BIG, da=(False, True)))
    return c


CASES = _build()
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def inputs(case):
    """-> dict(k, v [B,N,D], q, dupd1, dupd2 [B,K,D], dattn1, dattn2 [B,N,K]) in the case's dtype, seeded by its shape."""
    B, N, K, D = case.B, case.N, case.K, case.D
    dt = DTYPES[case.dtype]
    g = torch.Generator().manual_seed(1000003 * N + 1009 * K + D + B)
    scale = 7.0 if case.big else 1.0                                 # logits ~ N(0, scale^2): +-3 sigma is about +-20
    out = {"k": torch.randn(B, N, D, generator=g) * (scale * D ** -0.5), "v": torch.randn(B, N, D, generator=g),
           "q": torch.randn(B, K, D, generator=g), "dupd1": torch.randn(B, K, D, generator=g),
           "dupd2": torch.randn(B, K, D, generator=g), "dattn1": torch.randn(B, N, K, generator=g) * 0.1,
           "dattn2": torch.randn(B, N, K, generator=g) * 0.1}
    return {n: t.to(dt) for n, t in out.items()}
