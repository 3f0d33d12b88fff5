"""The slot-attention kernels (csrc/slot_attn.hip) by the C ABI against tests/slot_attn_ref.py in fp64: every route of
focus_slot_attn_fwd / focus_slot_attn_bwd / focus_slot_kv_grad (MFMA forward FULL and ragged, deferred backward with and
without a cotangent of attn_vis, slot_bwd_mfma_kernel at every D, the generic kernels in fp32 and bf16 at every KP and DV,
accumulate = 1, batch strides with gaps, a misaligned k_t, both eps, the row-count edges of the 256 / 64 / 32 / 16-row units).

Every buffer lives between two margins; outputs, margins, the workspace and the gaps between batch elements are pre-filled
with NaN bit patterns no kernel produces, and the workspace is exactly focus_slot_attn_workspace_bytes long.  After every
call: status OK, every margin and gap bit-identical, every output element finite (so: written), the inputs and the saved
forward tensors unchanged.  The backward is judged as a function of what it READ: the reference is evaluated on the
device's own stored attn_vis, colsum and updates.  Which kernel ran is asserted through focus_slot_attn_route.

With FOCUS_MARGINS set every test appends its largest error / magnitude per quantity; the figures measured on an MI355X and
the limits of the fp32 routes derived from them are the comment at the end of this file.

What these tests found: `updates` of slot_fwd_mfma_kernel missed U = 2^-8 of w^T |v| on seven cases with few rows
(ragged_n1 1.34 U, ragged_n15 1.51 U, ragged_n17 1.23 U, ragged_k16_d256 1.20 U, direct_n33_k16_d128 / d192 / d256 1.08 /
1.07 / 1.04 U).  The kernel rounded each weight (attn + eps) to bf16 as the MFMA operand of the row sum and
slot_fwd_finish rounds the quotient again; over hundreds of rows the operand roundings average out, with one or a few
dominant rows per slot they do not.  The kernel now feeds the rounding residue through a second MFMA on the same image
fragment, and every case holds the bound (the figures below are from the kernel as it is now)."""
import os

import pytest
import torch

import slot_attn_ref as sa
from test_gpu_kernels import RT, U, Check
from test_gpu_parity import TOL, dev
from test_gpu_traj_space import FILL, OK, Guarded, _stream
from test_slot_attn_ref_cpu import SWITCHES, routes

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
IDS = [c.name for c in sa.CASES]
# colsum is fp32: N terms accumulated in fp32, N * 2^-24 of sum |a + eps| (= colsum), plus the share of __expf and the
# reciprocal in every a (logits of +-20 times log2 e are rounded to fp32 before the exponential: about 40 * 2^-24 relative):
# 4 x the largest colsum error measured over the table, 1.03e-6 of colsum (see the end of the file)
COLSUM_EXPF = 4 * 1.03e-6
# fp32 routes: 4 x the largest measured error / magnitude, rounded up to a power of two (see the end of the file); the
# gradients of k and q against the TERM magnitudes of slot_attn_ref.backward
F32_LIM = {"attn": 2.0 ** -16, "upd": 2.0 ** -17, "dq": 2.0 ** -24, "dk": 2.0 ** -22, "dv": 2.0 ** -19, "dk_acc": 2.0 ** -22,
           "dv_acc": 2.0 ** -19, "ops_dq": 2.0 ** -25, "ops_dk": 2.0 ** -22, "ops_dv": 2.0 ** -20}
assert all(v <= TOL[torch.float32] for v in F32_LIM.values())


class Buf(Guarded):
    """B batch elements of `inner` elements, `bs` apart, starting `off` elements into the guarded area: what lies between
    them (and the `off` elements in front) keeps the fill."""

    def __init__(self, B, inner, bs, dtype, vals=None, off=0):
        super().__init__(off + (B - 1) * bs + inner, dtype)
        self.off = off
        self.shape = (B, inner)
        self.idx = (off + torch.arange(B, device=dev())[:, None] * bs + torch.arange(inner, device=dev())[None, :]).reshape(-1)
        self.gap = torch.ones(self.n, dtype=torch.bool, device=dev())
        self.gap[self.idx] = False
        if vals is not None:
            self.data()[self.idx] = vals.reshape(-1).to(dev())

    def ptr(self):
        p = self.data().data_ptr()
        assert p % 16 == 0
        return p + self.off * self.data().element_size()

    def get(self):
        return self.data()[self.idx].view(self.shape)

    def raw(self):
        return self.buf[self.m:self.m + self.n][self.idx].view(self.shape)

    def intact(self):
        return self.margins_intact() and bool((self.buf[self.m:self.m + self.n][self.gap] == self.fill).all())


def _refill(b):
    b.buf.fill_(b.fill)


def _structure(g, written, frozen, what):
    torch.cuda.synchronize()
    for n, b in g.items():
        assert b.intact() if isinstance(b, Buf) else b.margins_intact(), "%s: written outside %s" % (what, n)
    for n in written:
        assert bool(torch.isfinite(g[n].get().float()).all()), "%s: not fully written (or not finite): %s" % (what, n)
    for n, was in frozen.items():
        assert torch.equal(g[n].buf, was), "%s: changed %s" % (what, n)


def _zero(t):
    return bool((t == 0).all())


@pytest.mark.parametrize("case", sa.CASES, ids=IDS)
def test_slot_kernels_by_the_abi(case, monkeypatch):
    from focus_amd import _lib
    L = _lib.lib()
    if case.hand is not None:
        monkeypatch.setenv("FOCUS_SLOT_HAND", case.hand)
    else:
        monkeypatch.delenv("FOCUS_SLOT_HAND", raising=False)
    B, N, K, D, eps = case.B, case.N, case.K, case.D, case.eps
    dt, code, f32 = sa.DTYPES[case.dtype], (_lib.BF16 if case.dtype == "bf16" else _lib.F32), case.dtype == "f32"
    kv_bs, attn_bs = N * D + case.kv_gap, N * K + case.attn_gap
    x = sa.inputs(case)
    g = {"k": Buf(B, N * D, kv_bs, dt, x["k"], off=case.k_off), "v": Buf(B, N * D, kv_bs, dt, x["v"]),
         "q": Buf(B, K * D, K * D, dt, x["q"]), "dupd1": Buf(B, K * D, K * D, dt, x["dupd1"]),
         "dupd2": Buf(B, K * D, K * D, dt, x["dupd2"]), "dattn1": Buf(B, N * K, attn_bs, dt, x["dattn1"]),
         "dattn2": Buf(B, N * K, attn_bs, dt, x["dattn2"]),
         "attn": Buf(B, N * K, attn_bs, dt), "upd": Buf(B, K * D, K * D, dt), "colsum": Buf(B, K, K, F32),
         "dq1": Buf(B, K * D, K * D, dt), "dq2": Buf(B, K * D, K * D, dt)}
    if case.wl:
        g.update(wl1=Buf(B, N * 32, N * 32, BF16), wl2=Buf(B, N * 32, N * 32, BF16), dkv=Buf(B, N * 2 * D, N * 2 * D, BF16))
    else:
        g.update(dk=Buf(B, N * D, kv_bs, dt), dv=Buf(B, N * D, kv_bs, dt))
    nb = L.focus_slot_attn_workspace_bytes(B, N, K, D)
    g["ws"] = Guarded(nb, U8)
    # ---- the route ----
    ptrs = {n: g[n].ptr() for n in ("k", "v", "q")}
    ptrs.update({"wl": g["wl1"].ptr()} if case.wl else {"dk": g["dk"].ptr(), "dv": g["dv"].ptr()})
    fwd_route, bwd_route = routes(L, case, ptrs)
    print(case.name, "fwd", fwd_route, "bwd", bwd_route)
    if not any(os.environ.get(s) for s in SWITCHES):
        assert fwd_route == case.fwd and bwd_route == case.bwd, (fwd_route, case.fwd, bwd_route, case.bwd)
    inputs = ("k", "v", "q", "dupd1", "dupd2", "dattn1", "dattn2")
    frozen = {n: g[n].buf.clone() for n in inputs}
    # ---- forward ----
    rc = L.focus_slot_attn_fwd(g["k"].ptr(), g["v"].ptr(), kv_bs, g["q"].ptr(), g["attn"].ptr(), attn_bs, g["upd"].ptr(),
                               g["colsum"].ptr(), g["ws"].ptr(), nb, B, N, K, D, eps, code, _stream())
    assert rc == OK, ("forward", rc)
    _structure(g, ("attn", "upd", "colsum"), frozen, "forward")
    frozen.update({n: g[n].buf.clone() for n in ("attn", "upd", "colsum")})
    attn = g["attn"].get().view(B, N, K).cpu()
    upd = g["upd"].get().view(B, K, D).cpu()
    colsum = g["colsum"].get().view(B, K).cpu()
    attn_r, colsum_r, upd_r = sa.forward(x["k"], x["v"], x["q"], eps)
    w_r = (attn_r + eps) / colsum_r.unsqueeze(-2)
    ck = Check()
    if K == 1:
        assert torch.equal(attn.double(), torch.ones_like(attn_r))
    else:
        ck.tight(attn, attn_r, "attn_vis", rtol=F32_LIM["attn"] if f32 else 1.01 * U)
    ck.tight(upd, upd_r, "updates", rtol=F32_LIM["upd"] if f32 else U, mag=w_r.transpose(-1, -2) @ x["v"].double().abs())
    ck.tight(colsum, colsum_r, "colsum", rtol=N * 2.0 ** -24 + COLSUM_EXPF, floor=0.0)

    # ---- backward: two calls on the saved forward tensors ----
    def bwd(i, accumulate):
        _refill(g["ws"])
        da = g["dattn%d" % i].ptr() if case.da[i - 1] else None
        rc = L.focus_slot_attn_bwd(g["k"].ptr(), g["v"].ptr(), kv_bs, g["q"].ptr(), g["attn"].ptr(), attn_bs,
                                   g["colsum"].ptr(), g["upd"].ptr(), g["dupd%d" % i].ptr(), da,
                                   None if case.wl else g["dk"].ptr(), None if case.wl else g["dv"].ptr(), accumulate,
                                   g["dq%d" % i].ptr(), g["ws"].ptr(), nb, B, N, K, D, eps, code,
                                   g["wl%d" % i].ptr() if case.wl else None, _stream())
        assert rc == OK, ("backward", i, rc)
        _structure(g, ("dq%d" % i,) + (("wl%d" % i,) if case.wl else ("dk", "dv")), frozen, "backward %d" % i)
        return sa.backward(x["k"], x["v"], x["q"], attn, colsum, upd, x["dupd%d" % i], x["dattn%d" % i] if case.da[i - 1] else None, eps)

    def lim(name, bf):
        return F32_LIM[name] if f32 else bf

    mk, mq = ("mag_k_terms", "mag_q_terms") if f32 else ("mag_k", "mag_q")     # (slot_attn_ref.backward on the two)
    first = {}
    refs = []
    for i in (1, 2):
        r = bwd(i, i - 1)
        refs.append(r)
        tag = " (call %d%s)" % (i, ", dattn" if case.da[i - 1] else ", dattn NULL")
        dq = g["dq%d" % i].get().view(B, K, D).cpu()
        if K == 1:
            assert _zero(dq), "dq of a single slot"
        else:
            ck.tight(dq, r["dq"], "dq" + tag, rtol=lim("dq", RT), mag=r[mq])
        if case.wl:
            wl = g["wl%d" % i].get().view(B, N, 32).cpu()
            assert _zero(wl[..., K:16]) and _zero(wl[..., 16 + K:]), "wl columns of slots that do not exist"
            ck.tight(wl[..., :K], r["w"], "wl w" + tag, rtol=U)
            if K == 1:
                assert _zero(wl[..., 16]), "dlogits of a single slot"
            else:
                ck.tight(wl[..., 16:16 + K], r["dlogits"], "wl dlogits" + tag, rtol=U, mag=r["dlg"])
            continue
        dk, dv = (g[n].get().view(B, N, D).cpu() for n in ("dk", "dv"))
        if i == 1:
            first = {"dk": dk.double(), "dv": dv.double()}                 # (bf16: the stored, rounded first result)
            ck.tight(dv, r["dv"], "dv" + tag, rtol=lim("dv", RT), mag=r["mag_v"])
            if K == 1:
                assert _zero(dk), "dk of a single slot"
            else:
                ck.tight(dk, r["dk"], "dk" + tag, rtol=lim("dk", RT), mag=r[mk])
        else:
            ck.tight(dv, first["dv"] + r["dv"], "dv accumulate" + tag, rtol=lim("dv_acc", RT), mag=r["mag_v"] + first["dv"].abs())
            if K == 1:
                assert _zero(dk), "dk of a single slot"
            else:
                ck.tight(dk, first["dk"] + r["dk"], "dk accumulate" + tag, rtol=lim("dk_acc", RT),
                         mag=r[mk] + first["dk"].abs())
    # ---- deferred: dk, dv of both calls from their wl rows, [dk | dv] as ops passes them ----
    if case.wl:
        frozen.update({n: g[n].buf.clone() for n in ("wl1", "wl2", "dq1", "dq2")})
        p = g["dkv"].ptr()
        rc = L.focus_slot_kv_grad(g["wl1"].ptr(), g["wl2"].ptr(), None, None, g["q"].ptr(), g["q"].ptr(), None, None,
                                  g["dupd1"].ptr(), g["dupd2"].ptr(), None, None, 2, p, p + 2 * D, N * 2 * D, 2 * D, B, N, K, D,
                                  code, _stream())
        assert rc == OK, ("kv_grad", rc)
        _structure(g, ("dkv",), frozen, "kv_grad")
        dkv = g["dkv"].get().view(B, N, 2 * D).cpu()
        ck.tight(dkv[..., D:], refs[0]["dv"] + refs[1]["dv"], "dv (kv_grad)", rtol=1.5 * RT, mag=refs[0]["mag_v"] + refs[1]["mag_v"])
        if K == 1:
            assert _zero(dkv[..., :D]), "dk of a single slot"
        else:
            ck.tight(dkv[..., :D], refs[0]["dk"] + refs[1]["dk"], "dk (kv_grad)", rtol=1.5 * RT,
                     mag=refs[0]["mag_k"] + refs[1]["mag_k"])
    ck.done()


# focus_slot_kv_grad on its own: every iteration count, row pitch and layout of the two gradients
LAYOUTS = {"separate_ld_D": (False, lambda D: D), "halves_ld_2D": (True, lambda D: 2 * D),
           "halves_ld_2D+8": (True, lambda D: 2 * D + 8), "separate_ld_2D+8": (False, lambda D: 2 * D + 8)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_slot_kv_grad_by_the_abi(layout):
    from focus_amd import _lib
    L = _lib.lib()
    if not L.focus_slot_kv_grad_ok(16, 64, _lib.BF16, 1):
        pytest.skip("FOCUS_SLOT_KV_DEFER=0: the deferred gradient kernel is switched off in this environment")
    halves, ld_of = LAYOUTS[layout]
    B = 2
    ck = Check()
    for iters in (1, 2, 3, 4):
        for j, N in enumerate((1, 255, 256, 257)):
            D, K = (64, 128, 192, 256)[(iters + j) % 4], (1, 5, 11, 16)[(iters + 2 * j + j // 2) % 4]
            kv_ld = ld_of(D)
            kv_bs = N * kv_ld + 8                                           # a gap between the batch elements
            gen = torch.Generator().manual_seed(97 * iters + N + D)
            wls, qs, dus = [], [], []
            for _ in range(iters):
                wl = torch.zeros(B, N, 32)
                wl[..., :K] = torch.rand(B, N, K, generator=gen) * 0.1
                wl[..., 16:16 + K] = torch.randn(B, N, K, generator=gen) * 0.1
                wls.append(wl.bfloat16())
                qs.append(torch.randn(B, K, D, generator=gen).bfloat16())
                dus.append(torch.randn(B, K, D, generator=gen).bfloat16())
            g = {}
            for i in range(iters):
                g["wl%d" % i] = Buf(B, N * 32, N * 32, BF16, wls[i])
                g["q%d" % i], g["du%d" % i] = Buf(B, K * D, K * D, BF16, qs[i]), Buf(B, K * D, K * D, BF16, dus[i])
            frozen = {n: b.buf.clone() for n, b in g.items()}
            if halves:
                g["dkv"] = Buf(B, N * kv_ld, kv_bs, BF16)
                pk, pv = g["dkv"].ptr(), g["dkv"].ptr() + 2 * D
            else:
                g["dk"], g["dv"] = Buf(B, N * kv_ld, kv_bs, BF16), Buf(B, N * kv_ld, kv_bs, BF16)
                pk, pv = g["dk"].ptr(), g["dv"].ptr()
            ptr = lambda pre: [g[pre + str(i)].ptr() if i < iters else None for i in range(4)]
            rc = L.focus_slot_kv_grad(*ptr("wl"), *ptr("q"), *ptr("du"), iters, pk, pv, kv_bs, kv_ld, B, N, K, D, _lib.BF16,
                                      _stream())
            what = "iters %d N %d K %d D %d" % (iters, N, K, D)
            assert rc == OK, (what, rc)
            _structure(g, (), frozen, what)
            fill = FILL[BF16][1]
            if halves:
                raw, val = g["dkv"].raw().view(B, N, kv_ld), g["dkv"].get().view(B, N, kv_ld)
                assert bool((raw[..., 2 * D:] == fill).all()), what + ": padding columns written"
                dk, dv = val[..., :D], val[..., D:2 * D]
            else:
                outs = []
                for n in ("dk", "dv"):
                    raw = g[n].raw().view(B, N, kv_ld)
                    assert bool((raw[..., D:] == fill).all()), what + ": padding columns written"
                    outs.append(g[n].get().view(B, N, kv_ld)[..., :D])
                dk, dv = outs
            assert bool(torch.isfinite(dk.float()).all()) and bool(torch.isfinite(dv.float()).all()), what + ": not fully written"
            rk, rv, mk, mv = sa.kv_grad(wls, qs, dus)
            ck.tight(dk.cpu(), rk, "dk " + what, rtol=1.5 * RT, mag=mk)
            ck.tight(dv.cpu(), rv, "dv " + what, rtol=1.5 * RT, mag=mv)
    ck.done()


@pytest.mark.parametrize("dtype,iters,shape", [("bf16", 5, (2, 300, 5, 64)), ("f32", 2, (2, 130, 3, 64))])
def test_ops_shared_kv_grad_on_the_accumulate_path(dtype, iters, shape):
    """ops.slot_attn_step with one SlotKVGrad where focus_slot_kv_grad_ok says no (more than 4 iterations; fp32): the
    backward launches add into one buffer (accumulate = 1), and the bookkeeping of acc.total / acc.dk / pending decides which
    launch starts it and which node hands the sum to autograd.  Against fp64 autograd on the same values."""
    from focus_amd import _lib, ops
    B, N, K, D = shape
    dt, f32, eps = sa.DTYPES[dtype], dtype == "f32", sa.EPS_BIG
    assert not _lib.lib().focus_slot_kv_grad_ok(K, D, _lib.F32 if f32 else _lib.BF16, iters)
    gen = torch.Generator().manual_seed(iters + N)
    k, v = (torch.randn(B, N, D, generator=gen) * D ** -0.5).to(dt), torch.randn(B, N, D, generator=gen).to(dt)
    qs = [torch.randn(B, K, D, generator=gen).to(dt) for _ in range(iters)]
    cus = [torch.randn(B, K, D, generator=gen).to(dt) for _ in range(iters)]
    cas = [(torch.randn(B, N, K, generator=gen) * 0.1).to(dt) for _ in range(iters)]
    kr, vr = k.double().requires_grad_(), v.double().requires_grad_()
    qr = [q.double().requires_grad_() for q in qs]
    loss, mag_k, mag_v, mag_q = 0.0, 0.0, 0.0, []
    for i in range(iters):
        attn, colsum, upd = sa.forward(kr, vr, qr[i], eps)
        loss = loss + (upd * cus[i].double()).sum() + (attn * cas[i].double()).sum()
        with torch.no_grad():
            r = sa.backward(kr, vr, qr[i], attn, colsum, upd, cus[i], cas[i], eps)
        mag_k, mag_v = mag_k + r["mag_k_terms" if f32 else "mag_k"], mag_v + r["mag_v"]
        mag_q.append(r["mag_q_terms" if f32 else "mag_q"])
    loss.backward()
    d = dev()
    kg, vg = k.to(d).requires_grad_(), v.to(d).requires_grad_()
    qg = [q.to(d).requires_grad_() for q in qs]
    acc = ops.SlotKVGrad()
    lg = 0.0
    for i in range(iters):
        u2, a2 = ops.slot_attn_step(kg, vg, qg[i], eps, acc)
        lg = lg + (u2.float() * cus[i].to(d).float()).sum() + (a2.float() * cas[i].to(d).float()).sum()
    lg.backward()
    assert acc.pending == 0 and acc.total == 0 and acc.dk is None and not acc.items
    ck = Check()
    ck.tight(vg.grad.cpu(), vr.grad, "ops dv, %d iterations" % iters, rtol=F32_LIM["ops_dv"] if f32 else RT, mag=mag_v)
    ck.tight(kg.grad.cpu(), kr.grad, "ops dk, %d iterations" % iters, rtol=F32_LIM["ops_dk"] if f32 else RT, mag=mag_k)
    for i in range(iters):
        ck.tight(qg[i].grad.cpu(), qr[i].grad, "ops dq of iteration %d" % i, rtol=F32_LIM["ops_dq"] if f32 else RT, mag=mag_q[i])
    ck.done()


# Measured on an MI355X (FOCUS_MARGINS), largest |got - want| / max(|want|, mag, floor) per group of cases.
#
# bf16 routes, in units of U = 2^-8 (colsum: of colsum itself):
#
#   cases         attn_vis updates  colsum    dq    wl w  wl dlogits  dv    dk   dv acc dk acc  dv kv_grad dk kv_grad
#   limit           1.01    1.00   N 2^-24    2.00  1.00    1.00     2.00  2.00   2.00   2.00     3.00       3.00
#                                 + 4.12e-6
#   full_*          0.98    0.70   1.65e-7    0.32  1.00    0.91                                  1.83       0.92
#   nohand_*        0.98    0.28   7.20e-8    0.19  0.96    0.84                                  1.27       0.65
#   ragged_*        1.00    0.98   1.02e-6    1.38  0.99    0.96                                  1.87       1.30
#   direct_*        0.99    0.83   2.77e-7    0.83                   1.00  0.86   1.00   0.91
#   gaps_*          0.99    0.51   1.23e-7    0.17  0.99    0.84     0.99  0.81   0.99   0.85     1.40       0.66
#   gap4_generic    0.99    0.29   8.90e-8    0.16                   0.98  0.56   0.98   0.79
#   misaligned_k    0.98    0.30   1.06e-7    0.13                   0.94  0.55   0.95   0.63
#   bf16_*          0.96    0.64   1.26e-7    0.25                   0.93  0.65   0.97   0.79
#   test_slot_kv_grad_by_the_abi (limit 3.00): dk 1.00, dv 0.99 (exact bf16 inputs: one output rounding)
#   test_ops_shared_kv_grad_on_the_accumulate_path[bf16] (limit 2.00, 5 iterations): dv 1.88, dk 0.93, dq 0.10
#
# `updates` before the rounding residue went through the MFMA as well: ragged_* 1.51, direct_* 1.08 (the seven misses of the
# docstring); now the largest is ragged_n15 at 0.98, one output rounding near its worst case.  The largest colsum error of
# the whole table, 1.02e-6 of colsum (ragged_n15, logits of +-20; N * 2^-24 = 8.9e-7 is its accumulation allowance), is what
# COLSUM_EXPF = 4 x 1.03e-6 is taken from.  Close to their limit by construction (one rounding of a stored value):
# attn_vis, wl w, wl dlogits, dv of the direct backward.  dq of ragged_n1 and ragged_n15 (1.38, 1.19 of 2.00): with few
# input rows dupd . v - r nearly cancels, and the bf16 rounding of d logits is not averaged over rows.
#
# fp32 routes (f32_*; generic kernels), error / magnitude, dk and dq against the term magnitudes of slot_attn_ref.backward;
# limit = 4 x measured, rounded up to a power of two, never above TOL[float32] = 1e-3:
#
#   quantity        measured    limit
#   attn_vis        2.79e-06    2^-16 (1.53e-05)
#   updates         1.05e-06    2^-17 (7.63e-06)
#   colsum          8.31e-07    N 2^-24 + 4.12e-06 (as for bf16)
#   dq              1.09e-08    2^-24 (5.96e-08)
#   dv              4.40e-07    2^-19 (1.91e-06)
#   dk              3.35e-08    2^-22 (2.38e-07)
#   dv accumulate   3.62e-07    2^-19 (1.91e-06)
#   dk accumulate   3.76e-08    2^-22 (2.38e-07)
#   ops dv          1.91e-07    2^-20 (9.54e-07)      test_ops_shared_kv_grad_on_the_accumulate_path[f32], 2 iterations,
#   ops dk          3.45e-08    2^-22 (2.38e-07)      against fp64 autograd (not the stored forward)
#   ops dq          4.12e-09    2^-25 (2.98e-08)
#
# The largest fp32 figures come from f32_n63_k32_d256 and f32_n129_k16_d256 (logits of +-20 through __expf, 256-term dot
# products).  The kernels use no atomics: a rerun reproduces every figure.
# f32_n63_k32_d256 is the one shape whose generic backward asks for more than 64 KiB of dynamic LDS (66,816 bytes); the
# entry point raises the kernel's limit first, and the case passed on its first run.
