"""The composed attention route of ops.small_attention (_SmallAttnFn: two strided batched GEMMs around the row softmax of
csrc/softmax.hip, an optional dropout multiplier, four more GEMMs around focus_softmax_bwd) written plainly in fp64, and
a model of what its storage formats alone cost.  The checker of tests/test_gpu_attn_composed.py, itself checked without
a GPU by tests/test_attn_ref_cpu.py; the product never imports this, and this imports neither a GPU nor focus_amd.

  softmax_rows / softmax_rows_bwd   the comment at the top of softmax.hip, restated
  attention                         the formula, gradients by autograd
  attention_rounded                 the same formula with a round trip through the storage dtype wherever the composed
                                    route keeps a tensor in memory; backward written out by hand
  CASES / inputs                    the table and the tensors both test files walk
"""
import zlib

import torch

# err(kernel, exact) <= max(FLOOR, FACTOR * err(model, exact)), and FACTOR * err(model, exact) <= CAP on every row of CASES.
# FLOOR is what test_small_attention_one_launch (tests/test_gpu_steve.py) holds the one-launch route to.
FLOOR = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -6}
CAP = {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -4}
# Not derived: it pays for what the model leaves out (fp32 accumulation order, the fast exponential).  Measured on an
# MI355X (table at the end of test_gpu_attn_composed.py): err(kernel, exact) / err(model, exact) is 1.000 on every bf16
# row, the only rows where this term and not FLOOR decides; up to 32.7 on the fp32 rows, all of them under FLOOR.
FACTOR = 4.0


def rt(t, dtype):
    """Round trip of fp64 values through the storage dtype (float64: no rounding)."""
    return t if dtype == torch.float64 else t.to(dtype).double()


def err(a, b):
    """max|a - b| / max|b|."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def softmax_rows(x, scale, period=None):
    """fp64 softmax(scale * x) over the last axis.  With `period`, row r (counted over all leading axes) sees columns
    0 .. r % period; the rest is exactly 0 whatever x holds there."""
    x = x.double()
    L = x.shape[-1]
    z = (scale * x).reshape(-1, L)
    if period is not None:
        r = torch.arange(z.shape[0], device=x.device)
        hidden = torch.arange(L, device=x.device)[None, :] > (r % period)[:, None]
        z = z.masked_fill(hidden, float("-inf"))
    e = torch.exp(z - z.max(-1, keepdim=True).values)           # exp(-inf) is exactly 0
    return (e / e.sum(-1, keepdim=True)).reshape(x.shape)


def softmax_rows_bwd(dy, y, scale):
    """dx = scale * y * (dy - sum(dy * y))."""
    dy, y = dy.double(), y.double()
    return scale * y * (dy - (dy * y).sum(-1, keepdim=True))


def _heads(t, heads):
    B, n, C = t.shape
    return t.view(B, n, heads, C // heads).transpose(1, 2)


def _rows(t):
    B, h, n, d = t.shape
    return t.transpose(1, 2).reshape(B, n, h * d)


def attention(q, k, v, heads, scale, causal, drop, cu):
    """fp64 attention on [B, n, C] rows, heads as column blocks; drop: [B, heads, Nq, Nk] multiplier on the
    probabilities or None.  -> (out, dq, dk, dv) of sum(out * cu)."""
    Nq, Nk = q.shape[1], k.shape[1]
    qd, kd, vd = (t.double().detach().requires_grad_() for t in (q, k, v))
    att = (_heads(qd, heads) * scale) @ _heads(kd, heads).transpose(-1, -2)
    if causal:
        assert Nq == Nk, "causal self-attention"
        att = att.masked_fill(torch.triu(torch.ones(Nq, Nk, dtype=torch.bool, device=q.device), diagonal=1), float("-inf"))
    att = torch.softmax(att, dim=-1)
    if drop is not None:
        att = att * drop.double()
    out = _rows(att @ _heads(vd, heads))
    (out * cu.double()).sum().backward()
    return out.detach(), qd.grad, kd.grad, vd.grad


def attention_rounded(q, k, v, heads, scale, causal, drop, cu, dtype):
    """attention() with every tensor the composed route stores rounded to `dtype`: the unscaled logits, the
    probabilities, probabilities * drop, out; dA = dO v^T, dA * drop, the softmax backward, dq, dk, dv.  Everything
    between two stores is fp64.  A model of the storage format, not of the kernels."""
    Nq, Nk = q.shape[1], k.shape[1]
    r = lambda t: rt(t, dtype)
    qh, kh, vh, do = (_heads(t.double(), heads) for t in (q, k, v, cu))
    if causal:
        assert Nq == Nk, "causal self-attention"
    logits = r(qh @ kh.transpose(-1, -2))
    p = r(softmax_rows(logits, scale, Nq if causal else None))
    pd = p if drop is None else r(p * drop.double())
    out = r(_rows(pd @ vh))
    da = r(do @ vh.transpose(-1, -2))
    if drop is not None:
        da = r(da * drop.double())
    ds = r(softmax_rows_bwd(da, p, scale))
    dq = r(_rows(ds @ kh))
    dk = r(_rows(ds.transpose(-1, -2) @ qh))
    dv = r(_rows(pd.transpose(-1, -2) @ do))
    return out, dq, dk, dv


F32, BF16 = torch.float32, torch.bfloat16
KEYS = ("B", "heads", "Nq", "Nk", "d", "dtype", "causal", "p", "layout", "gain")
# layout: "dense" | "qkv" (q, k, v are the column blocks of one [B, n, 3C] buffer) | "cu_view" (the cotangent is a
# non-contiguous view).  gain: the factor on randn for q and k.
CASES = [dict(zip(KEYS, row)) for row in [
    (2, 4, 1024, 1024, 48, F32, True, 0.0, "dense", 0.7),      # STEVE decoder self-attention, fp32
    (2, 4, 1024, 1024, 48, F32, True, 0.1, "dense", 0.7),      # ... in training
    (2, 4, 1024, 11, 48, F32, False, 0.1, "dense", 0.7),       # decoder cross-attention to the slots: row shorter than a wave
    (3, 3, 77, 77, 24, BF16, True, 0.25, "qkv", 0.7),          # head width flash turns down; strided inputs copied
    (2, 2, 5, 5, 96, BF16, False, 0.0, "dense", 0.7),          # wider than the one-launch limit
    (32, 4, 11, 11, 48, F32, True, 0.0, "dense", 0.7),         # one-launch shape sent to the composed route by the mask
    (32, 4, 11, 11, 48, BF16, False, 0.1, "dense", 0.7),       # ... by the dropout mask
    (1, 2, 785, 197, 96, F32, False, 0.0, "dense", 0.7),       # MViT pooled attention: Nq != Nk, ragged on both sides
    (1, 1, 129, 129, 8, BF16, True, 0.0, "cu_view", 0.7),      # L = 2 * 64 + 1; dout.contiguous()
]]


def case_id(c):
    return "%dx%dx%dx%dx%d-%s%s%s-%s" % (c["B"], c["heads"], c["Nq"], c["Nk"], c["d"],
                                         "bf16" if c["dtype"] == BF16 else "fp32", "-causal" if c["causal"] else "",
                                         "-p%g" % c["p"] if c["p"] else "", c["layout"])


def inputs(c):
    """-> q, k, v, cu, drop (None when p == 0) on the CPU in the case's dtype; scale.  Seeded by the row itself."""
    B, h, Nq, Nk, C, dt = c["B"], c["heads"], c["Nq"], c["Nk"], c["heads"] * c["d"], c["dtype"]
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    q = (torch.randn(B, Nq, C, generator=g) * c["gain"]).to(dt)
    k = (torch.randn(B, Nk, C, generator=g) * c["gain"]).to(dt)
    v = torch.randn(B, Nk, C, generator=g).to(dt)
    cu = torch.randn(B, Nq, C, generator=g).to(dt)
    drop = None
    if c["p"] > 0:
        drop = (torch.bernoulli(torch.full((B, h, Nq, Nk), 1.0 - c["p"]), generator=g) / (1.0 - c["p"])).to(dt)
    return q, k, v, cu, drop, c["d"] ** -0.5
