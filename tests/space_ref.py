"""The fused space step of trajectory attention (csrc/traj_space_mfma.hip, traj_space_bwd_mfma.hip, traj_cls.hip; bf16, head
dim 64) written plainly in fp64, a model of where those kernels round, the magnitudes and counted limits the kernels are
held to, the case table, and small wrong variants of the model.  The checker of tests/test_gpu_traj_space.py, itself
checked without a GPU by tests/test_space_ref_cpu.py; the product never imports this, and this imports neither a GPU nor
focus_amd.

  space_exact      attention.py:509-535 in fp64, d(qkv) by autograd, and the magnitudes below
  space_rounded    the same formula with a bf16 round trip exactly where the fused kernels round; backward by hand
  quantities       the checked parts of a result with their magnitude, limit and floor
  CASES / inputs   the table and the tensors both test files walk
  MUTANTS          wrong variants of space_rounded (CPU only): what the limits are there to catch
  tiling / route   focus_traj_space_tiling and the kernel instantiations a row reaches, restated

Magnitudes (per element; A = the frame softmax, dX = d(x~) + [own frame] d(x_diag)):
  mag_x  = sum_p A |v|
  E      = A * scale * (sum_d |dX||v_p| + sum_d |dX||x~|)      the UNCANCELLED size of dL = A (dP - delta) scale: it covers
           the cancellation in dP - delta and the error delta inherits from the bf16-stored x~, and stays positive at
           P = 1 where the exact dQ and dK are 0
  mag_dq = sum_{f,p} E |k|      mag_dk = sum_s E |q| + |cls-row part of dK|      mag_dv = sum_s A |dX| + |cls-row part of dV|

Limits: every rounding costs at most U = 2^-8 of its magnitude; 1 % is the allowance for fp32 summation order.
  x~, x_diag   2 roundings: the un-normalised probabilities as the P.V operand, the output
  dQ           2: dL as the operand, the output (delta's error sits inside E)
  dK, dV       3: the operand (dL / P), the patch kernel's output, the output again after the cls row's part is added
  cls_out and the token-0 row of dqkv: fp32 arithmetic, one output rounding
These are constants, not fitted to a GPU result.  (space_rounded also rounds the own-frame dX row d(x~) + d(x_diag) the way
traj_dxsum_kernel stores it: one query's term in F of the sums above, not counted as a rounding of its own;
test_space_ref_cpu.py shows the whole model inside the limits on every row of the table.)
"""
import math
import zlib

import torch

U = 2.0 ** -8
LIM_X = 2.02 * U
LIM_DQ = 2.02 * U
LIM_DKV = 3.03 * U
LIM_CLS = 1.01 * U
FLOOR_CLS = 1e-2          # Check.tight's own floor, for the cls quantities only: the others are held to max(|want|, mag)
HD = 64
MAX_KEY_BLOCKS = 14       # FOCUS_TRAJ_MAX_KEY_BLOCKS
MAXF = 16                 # frames the backward's per-wave lse table holds


def r16(t):
    """Round trip of fp64 values through bf16 (round to nearest even)."""
    return t.float().bfloat16().double()


def _same(t):
    return t


def tiling(P):
    """focus_traj_space_tiling: ceil(P/32) key blocks = NT tiles of NKB blocks, NKB <= 7 the largest divisor."""
    nb = (P + 31) // 32
    k = min(nb, 7)
    while nb % k:
        k -= 1
    return k, nb // k


def route(case):
    """What the dispatchers pick for a row: forward (NKB, MULTI), dQ NB, dK/dV NKB; dQ stream length, query chunks of
    dK/dV, and the workgroup counts of the three grids."""
    _, B, heads, F, P = case
    nkb, nt = tiling(P)
    nb, S = (P + 31) // 32, F * P
    qt = (S + 127) // 128
    return {"fwd": (nkb, nt > 1), "dq": nb, "dkv": nkb, "stream": F * nb, "chunks": (S + 31) // 32,
            "grids": (qt * B * heads, F * nt * B * heads)}


def _heads(t, heads):                         # [B,n,(h d)] -> [B,h,n,d]
    B, n, C = t.shape
    return t.reshape(B, n, heads, C // heads).permute(0, 2, 1, 3)


def _merge(t):                                # [B,h,n,d] -> [B,n,(h d)]
    B, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, h * d)


def _merge_f(t):                              # [B,h,S,F,d] -> [B,S,F,(h d)]
    B, h, S, F, d = t.shape
    return t.permute(0, 2, 3, 1, 4).reshape(B, S, F, h * d)


def _split_f(t, heads):                       # [B,S,F,(h d)] -> [B,h,S,F,d]
    B, S, F, C = t.shape
    return t.reshape(B, S, F, heads, C // heads).permute(0, 3, 1, 2, 4)


def _own(S, F, P, shift=0):
    """own[s, f]: frame f is query s's own frame.  shift = 1 is mutant (e)."""
    fs = torch.clamp((torch.arange(S) + shift) // P, max=F - 1)
    return fs, fs[:, None] == torch.arange(F)[None, :]


def _cls(q, k, v, dc, scale):
    """The cls query row over all N keys, forward and backward, in fp64: (cls [B,h,d], dq0 [B,h,d], the cls row's parts
    of dK and dV [B,h,N,d])."""
    q0 = q[:, :, 0]
    a = torch.softmax(scale * torch.einsum("bhd,bhnd->bhn", q0, k), dim=-1)
    cls = torch.einsum("bhn,bhnd->bhd", a, v)
    da = torch.einsum("bhd,bhnd->bhn", dc, v)
    dl = scale * a * (da - (a * da).sum(-1, keepdim=True))
    return cls, torch.einsum("bhn,bhnd->bhd", dl, k), dl[..., None] * q0[:, :, None, :], a[..., None] * dc[:, :, None, :]


def space_exact(qkv, F, P, heads, cts):
    """attention.py:509-535 in fp64 on the given values.  -> dict: xt [B,S,F,C], xd [B,S,C], cls [B,1,C], dqkv [B,N,3C] by
    autograd for the cotangents cts = (dxt, dxdiag, dcls), and mag_x, mag_xd, mag_dq, mag_dk, mag_dv."""
    B, N, C3 = qkv.shape
    C, S = C3 // 3, F * P
    d = C // heads
    scale = d ** -0.5
    cts = [c.double() for c in cts]
    q64 = qkv.double().requires_grad_()
    q, k, v = (_heads(t, heads) for t in q64.split(C, dim=-1))
    cls = _merge(torch.softmax((q[:, :, :1] * scale) @ k.transpose(-1, -2), dim=-1) @ v)
    A = torch.softmax((q[:, :, 1:] @ k[:, :, 1:].transpose(-1, -2)).reshape(B, heads, S, F, P) * scale, dim=-1)
    vf = v[:, :, 1:].reshape(B, heads, F, P, d)
    xh = torch.einsum("bhsfp,bhfpd->bhsfd", A, vf)
    xt = _merge_f(xh)
    fs, own = _own(S, F, P)
    xd = xt[:, torch.arange(S), fs]
    ((xt * cts[0]).sum() + (xd * cts[1]).sum() + (cls * cts[2]).sum()).backward()
    with torch.no_grad():
        mag_x = _merge_f(torch.einsum("bhsfp,bhfpd->bhsfd", A, vf.abs()))
        dX = cts[0].clone()
        dX[:, torch.arange(S), fs] += cts[1]
        dXh = _split_f(dX, heads).abs()
        E = A * scale * (torch.einsum("bhsfd,bhfpd->bhsfp", dXh, vf.abs()) + (dXh * xh.abs()).sum(-1, keepdim=True))
        kf, qs = k[:, :, 1:].reshape(B, heads, F, P, d), q[:, :, 1:]
        _, _, dk_c, dv_c = _cls(q, k, v, _heads(cts[2], heads)[:, :, 0], scale)
        mag_dq = _merge(torch.einsum("bhsfp,bhfpd->bhsd", E, kf.abs()))
        mag_dk = _merge(torch.einsum("bhsfp,bhsd->bhfpd", E, qs.abs()).reshape(B, heads, S, d) + dk_c[:, :, 1:].abs())
        mag_dv = _merge(torch.einsum("bhsfp,bhsfd->bhfpd", A, dXh).reshape(B, heads, S, d) + dv_c[:, :, 1:].abs())
    return {"xt": xt.detach(), "xd": xd.detach(), "cls": cls.detach(), "dqkv": q64.grad, "mag_x": mag_x,
            "mag_xd": mag_x[:, torch.arange(S), fs], "mag_dq": mag_dq, "mag_dk": mag_dk, "mag_dv": mag_dv}


# what each mutant gets wrong, and the rows it applies to (case -> bool)
MUTANTS = {
    "fwd_pad_key_kept": lambda c: True,                       # (a) one padded key, a copy of the last, in the forward softmax
    "fwd_last_key_dropped": lambda c: c[4] > 1,               # (b)
    "dq_pad_key_kept": lambda c: c[4] > 1,                    # (c) the same two in dQ's key stream; at P = 1 dL is exactly 0
    "dq_last_key_dropped": lambda c: c[4] > 1,
    "merge_without_rescale": lambda c: tiling(c[4])[1] > 1,   # (d) a later key tile merged onto an un-rescaled accumulation
    "frame_owner_off_by_one": lambda c: c[3] > 1,             # (e) x_diag and the dX-sum row at a frame boundary
    "pad_queries_reach_dkv": lambda c: (c[3] * c[4]) % 32 != 0,   # (f) copies of row S-1 in the last 32-query chunk
}


def space_rounded(qkv, F, P, heads, cts, rounding=True, mutant=None):
    """space_exact's formula evaluated the way the fused kernels evaluate it, fp64 between the points where they round to
    bf16:  the un-normalised exp(l - max) as the P.V operand (per key tile, against the running max, when the frame is
    tiled) and the output;  the own-frame dX row d(x~) + d(x_diag) (traj_dxsum_kernel);  delta from the STORED x~;  dL as
    the operand of dQ and dK, P as the operand of dV;  dQ once;  dK / dV once by the patch kernel and again after the cls
    row's part is added (cls_bwd_b_kernel);  cls_out and the token-0 row once.  -> dict: xt, xd, cls, dqkv."""
    assert mutant is None or mutant in MUTANTS
    r = r16 if rounding else _same
    B, N, C3 = qkv.shape
    C, S = C3 // 3, F * P
    d = C // heads
    scale = d ** -0.5
    q, k, v = (_heads(t, heads) for t in qkv.double().split(C, dim=-1))
    qs = q[:, :, 1:]
    kf, vf = k[:, :, 1:].reshape(B, heads, F, P, d), v[:, :, 1:].reshape(B, heads, F, P, d)
    L = torch.einsum("bhsd,bhfpd->bhsfp", qs, kf) * scale
    # ---- forward: key tiles of NKB * 32 keys merged by an online softmax ----
    Lf, vff = L, vf
    if mutant == "fwd_pad_key_kept":
        Lf, vff = torch.cat([L, L[..., -1:]], -1), torch.cat([vf, vf[..., -1:, :]], -2)
    elif mutant == "fwd_last_key_dropped":
        Lf, vff = L[..., :-1], vf[..., :-1, :]
    nkb, nt = tiling(P)
    m_run = ssum = y = None
    for j in range(nt):
        sl = slice(j * nkb * 32, (j + 1) * nkb * 32 if j + 1 < nt else None)
        m = Lf[..., sl].max(-1).values
        if j == 0:
            m_run = m
            pe = torch.exp(Lf[..., sl] - m_run[..., None])
            ssum = pe.sum(-1)
            y = torch.einsum("bhsfp,bhfpd->bhsfd", r(pe), vff[..., sl, :])
        else:
            m_new = torch.maximum(m_run, m)
            alpha = torch.exp(m_run - m_new) if mutant != "merge_without_rescale" else torch.ones_like(m)
            m_run = m_new
            pe = torch.exp(Lf[..., sl] - m_run[..., None])
            ssum = ssum * alpha + pe.sum(-1)
            y = y * alpha[..., None] + torch.einsum("bhsfp,bhfpd->bhsfd", r(pe), vff[..., sl, :])
    xh = r(y / ssum[..., None])                                   # the stored x~ [B,h,S,F,d]
    lse = m_run + torch.log(ssum)
    fs, own = _own(S, F, P, 1 if mutant == "frame_owner_off_by_one" else 0)
    xt = _merge_f(xh)
    xd = xt[:, torch.arange(S), fs]
    # ---- backward of the patch rows ----
    dxt, dxd = _split_f(cts[0].double(), heads), _heads(cts[1].double(), heads)
    dX = torch.where(own[None, None, :, :, None], r(dxt + dxd[:, :, :, None, :]), dxt)
    delta = scale * (dX * xh).sum(-1)
    Pm = torch.exp(L - lse[..., None])
    dL = Pm * (torch.einsum("bhsfd,bhfpd->bhsfp", dX, vf) * scale - delta[..., None])
    dLr, Pr = r(dL), r(Pm)
    dq = torch.einsum("bhsfp,bhfpd->bhsd", dLr, kf)
    if mutant in ("dq_pad_key_kept", "dq_last_key_dropped"):
        extra = torch.einsum("bhsf,bhfd->bhsd", dLr[..., -1], kf[..., -1, :])
        dq = dq + extra if mutant == "dq_pad_key_kept" else dq - extra
    dk = torch.einsum("bhsfp,bhsd->bhfpd", dLr, qs)
    dv = torch.einsum("bhsfp,bhsfd->bhfpd", Pr, dX)
    if mutant == "pad_queries_reach_dkv":
        npad = -S % 32
        dk = dk + npad * dLr[:, :, -1, :, :, None] * qs[:, :, -1, None, None, :]
        dv = dv + npad * Pr[:, :, -1, :, :, None] * dX[:, :, -1, :, None, :]
    dq, dk, dv = r(dq), r(dk).reshape(B, heads, S, d), r(dv).reshape(B, heads, S, d)
    # ---- cls row: fp32 arithmetic throughout; its parts of dK / dV are added onto the stored patch rows ----
    cls, dq0, dk_c, dv_c = _cls(q, k, v, _heads(cts[2].double(), heads)[:, :, 0], scale)
    parts = [torch.cat([r(dq0)[:, :, None], dq], 2), r(torch.cat([dk_c[:, :, :1], dk + dk_c[:, :, 1:]], 2)),
             r(torch.cat([dv_c[:, :, :1], dv + dv_c[:, :, 1:]], 2))]
    dqkv = torch.cat([_merge(t) for t in parts], -1)
    return {"xt": xt, "xd": xd, "cls": r(_merge(cls[:, :, None])), "dqkv": dqkv}


def quantities(got, ref):
    """The checked parts: (what, got, want, mag or None, limit, floor).  |got - want| <= limit * max(|want|, mag,
    floor * max|want|) per element -- Check.tight of tests/test_gpu_kernels.py."""
    C = ref["xd"].shape[-1]
    g, w = got["dqkv"], ref["dqkv"]
    return [("x~ (traj_space_fwd)", got["xt"], ref["xt"], ref["mag_x"], LIM_X, 0.0),
            ("x_diag (traj_space_fwd)", got["xd"], ref["xd"], ref["mag_xd"], LIM_X, 0.0),
            ("cls_out (cls_fwd)", got["cls"], ref["cls"], None, LIM_CLS, FLOOR_CLS),
            ("dQ patch rows (traj_dq)", g[:, 1:, :C], w[:, 1:, :C], ref["mag_dq"], LIM_DQ, 0.0),
            ("dK patch rows (traj_dkv + cls_bwd)", g[:, 1:, C:2 * C], w[:, 1:, C:2 * C], ref["mag_dk"], LIM_DKV, 0.0),
            ("dV patch rows (traj_dkv + cls_bwd)", g[:, 1:, 2 * C:], w[:, 1:, 2 * C:], ref["mag_dv"], LIM_DKV, 0.0),
            ("token-0 row of dqkv (cls_bwd)", g[:, :1], w[:, :1], None, LIM_CLS, FLOOR_CLS)]


def ratio(got, want, mag=None, floor=0.0):
    """max over the elements of |got - want| / max(|want|, mag, floor * max|want|): Check.tight's figure."""
    want, got = want.double(), got.double()
    den = torch.clamp(want.abs(), min=floor * float(want.abs().max()))
    if mag is not None:
        den = torch.maximum(den, mag.double().abs())
    return float(((got - want).abs() / den).max()) if bool(torch.isfinite(got).all()) else float("inf")


# (id, B, heads, F, P); bf16, head dim 64.  Every key-block count 1..14 occurs with B >= 2 and with heads in {1, 3}.
CASES = [
    # key blocks 1..7 in one tile, ragged and full
    ("p1", 2, 3, 1, 1), ("p2", 2, 1, 3, 2), ("p31", 2, 3, 2, 31), ("p32_s128", 1, 2, 4, 32),
    ("p33", 2, 3, 2, 33), ("p64", 1, 2, 2, 64), ("p65", 2, 1, 2, 65), ("p96", 1, 3, 3, 96),
    ("p97_f5", 2, 1, 5, 97), ("p129", 2, 3, 2, 129), ("p160", 1, 1, 3, 160), ("p190", 2, 1, 2, 190),
    ("p196", 2, 3, 2, 196), ("p224", 1, 2, 3, 224),
    # 8..14 blocks: tiles merged by the online softmax (2x4, 3x3, 2x5, 11x1, 2x6, 13x1, 2x7)
    ("p225", 2, 1, 2, 225), ("p270", 1, 1, 2, 270), ("p288", 2, 3, 2, 288), ("p300", 2, 1, 2, 300), ("p330", 2, 1, 2, 330),
    ("p352", 1, 3, 2, 352), ("p353", 2, 1, 2, 353), ("p384", 1, 3, 2, 384), ("p390", 2, 1, 2, 390),
    ("p416", 1, 3, 2, 416), ("p417", 2, 1, 2, 417), ("p447", 1, 3, 2, 447), ("p448", 2, 1, 2, 448),
    # streams shorter than the rings: F = 1 (dQ stream of 1, 2, 3 steps), S = 30, 50, 90, 129
    ("f1_p20", 2, 3, 1, 20), ("f1_p40", 2, 1, 1, 40), ("f1_p70", 1, 3, 1, 70),
    ("s30", 1, 1, 2, 15), ("s50", 2, 2, 2, 25), ("s90", 1, 3, 3, 30), ("s129", 2, 1, 3, 43),
    # F = 16: the whole lse table of the backward
    ("f16_p5", 2, 3, 16, 5), ("f16_p33", 1, 1, 16, 33),
]


def _hadamard_row(i):
    """Row i of the 64 x 64 Sylvester matrix over 8: a unit vector, exact in bf16, orthogonal to the other rows."""
    return torch.tensor([(-1.0) ** bin(i & j).count("1") for j in range(HD)]) / 8.0


def inputs(case):
    """(qkv [B,N,3C], (dxt, dxdiag, dcls)) of a row, bf16 on the CPU, seeded from the row's id.  randn, and on top of it
    (P > 1; directions are orthogonal unit vectors, the same in every head):
      * the frame's LAST real key (index P-1 of every frame) is 4 u, and every third query (s % 3 == 0) is shifted by
        2 ln(P-1) u: that key's logit gains ln(P-1) and it holds ~0.15-0.5 of the frame's mass -- a wrong tail mask moves
        those rows by a multiple of the limit at every P;
      * tiled rows (P > 224): the frame's FIRST key is 4 u2 and the queries s % 3 == 1 are shifted by 2 (ln(P-1) + 2) u2, so
        their largest logit sits in the first key tile and the spiked third's in the last: the merge sees alpha < 1 in
        both orders;
      * the LAST query is shifted by 2 (ln P + 3) u3 towards key min(1, P-2) of every frame, 4 u3, which no other query
        favours: a copy of the last query's row leaking into dK / dV is a multiple of that key's magnitude.
    Logit gaps stay below ~40."""
    name, B, heads, F, P = case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    C, S = heads * HD, F * P
    qkv = torch.randn(B, 1 + S, 3, heads, HD, generator=g)
    if P > 1:
        u, u2, u3 = _hadamard_row(1), _hadamard_row(2), _hadamard_row(3)
        s = torch.arange(S)
        tok = 1 + s.reshape(F, P)                                   # token index of (frame, key)
        qkv[:, tok[:, P - 1], 1] = 4 * u
        qkv[:, 1 + s[s % 3 == 0], 0] += 2 * math.log(P - 1) * u
        if tiling(P)[1] > 1:
            qkv[:, tok[:, 0], 1] = 4 * u2
            qkv[:, 1 + s[s % 3 == 1], 0] += 2 * (math.log(P - 1) + 2) * u2
        qkv[:, tok[:, min(1, P - 2)], 1] = 4 * u3
        qkv[:, S, 0] = torch.randn(B, heads, HD, generator=g) + 2 * (math.log(P) + 3) * u3
    qkv = qkv.reshape(B, 1 + S, 3 * C).bfloat16()
    cts = (torch.randn(B, S, F, C, generator=g).bfloat16(), torch.randn(B, S, C, generator=g).bfloat16(),
           torch.randn(B, 1, C, generator=g).bfloat16())
    return qkv, cts
