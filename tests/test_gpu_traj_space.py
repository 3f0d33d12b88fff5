"""The fused space-attention kernels (csrc/traj_space_mfma.hip, traj_space_bwd_mfma.hip, traj_cls.hip) by the C ABI against
tests/space_ref.py in fp64: every key-block count and key tiling, ragged and full last blocks, B > 1, odd head counts,
F = 1 and F = 16, streams shorter than the DMA rings, S from 1 to 1344.

Every buffer (inputs, cotangents, outputs, the fp32 tables, the workspace) lives inside a larger one with a margin in front
and behind; outputs, margins and the workspace are pre-filled with NaN bit patterns no kernel produces, and the workspace
is exactly focus_traj_space_workspace_bytes long.  After forward and backward every margin is bit-identical, every output
element is finite (so: written), the inputs and the saved x~ are unchanged, and every element is held to the counted
limits of space_ref.py (checked without a GPU, with the case table, in test_space_ref_cpu.py).

With FOCUS_MARGINS set every test appends its largest error / magnitude per quantity; the figures measured on an MI355X
are the comment at the end of this file."""
import ctypes
import os

import pytest
import torch

import space_ref as sr
from test_gpu_kernels import Check
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
FILL = {BF16: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC00123), U8: (torch.uint8, 0xFF)}   # NaNs no kernel produces
MARGIN = 256                                                     # bytes in front and behind; keeps the data 16-byte aligned
OK = 0


class Guarded:
    """n elements of dtype between two pre-filled margins; vals (optional) fill the n."""

    def __init__(self, n, dtype, vals=None):
        it, fill = FILL[dtype]
        self.m = MARGIN // torch.empty(0, dtype=it).element_size()
        self.n, self.dtype, self.fill = n, dtype, fill
        self.buf = torch.full((2 * self.m + n,), fill, device=dev(), dtype=it)
        if vals is not None:
            self.data().copy_(vals.reshape(-1))

    def data(self):
        return self.buf[self.m:self.m + self.n].view(self.dtype)

    def ptr(self):
        assert self.data().data_ptr() % 16 == 0
        return self.data().data_ptr()

    def margins_intact(self):
        return bool((self.buf[:self.m] == self.fill).all()) and bool((self.buf[self.m + self.n:] == self.fill).all())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fused_or_skip():
    if os.environ.get("FOCUS_TRAJ_FUSED", "1").strip() == "0":
        pytest.skip("FOCUS_TRAJ_FUSED=0: the fused space-attention kernels are switched off in this environment")


def run_abi(case, qkv, cts):
    """Forward and backward of one row by the C ABI inside guarded buffers.  -> (outputs on the CPU, workspace bytes)."""
    from focus_amd import _lib
    L = _lib.lib()
    _, B, heads, F, P = case
    S, C = F * P, heads * sr.HD
    dims = (B, F, P, heads, sr.HD, _lib.BF16)
    g = {"qkv": Guarded(qkv.numel(), BF16, qkv.to(dev())), "dxt": Guarded(cts[0].numel(), BF16, cts[0].to(dev())),
         "dxdiag": Guarded(cts[1].numel(), BF16, cts[1].to(dev())), "dcls": Guarded(cts[2].numel(), BF16, cts[2].to(dev())),
         "xt": Guarded(B * S * F * C, BF16), "xdiag": Guarded(B * S * C, BF16), "cls_out": Guarded(B * C, BF16),
         "lse": Guarded(B * heads * S * F, F32), "cls_lse": Guarded(B * heads, F32), "dqkv": Guarded(qkv.numel(), BF16)}
    nf, nb = (L.focus_traj_space_workspace_bytes(*dims, bw) for bw in (0, 1))
    g["ws_fwd"], g["ws_bwd"] = Guarded(nf, U8), Guarded(nb, U8)
    rc = L.focus_traj_space_fwd(g["qkv"].ptr(), g["xt"].ptr(), g["xdiag"].ptr(), g["cls_out"].ptr(), g["lse"].ptr(),
                                g["cls_lse"].ptr(), g["ws_fwd"].ptr(), nf, *dims, _stream())
    torch.cuda.synchronize()
    assert rc == OK, ("forward", rc)
    saved = {k: g[k].data().view(FILL[g[k].dtype][0]).clone() for k in ("xt", "lse", "cls_lse", "cls_out", "xdiag")}
    rc = L.focus_traj_space_bwd(g["qkv"].ptr(), g["xt"].ptr(), g["cls_out"].ptr(), g["lse"].ptr(), g["cls_lse"].ptr(),
                                g["dxt"].ptr(), g["dxdiag"].ptr(), g["dcls"].ptr(), g["dqkv"].ptr(), g["ws_bwd"].ptr(), nb,
                                *dims, _stream())
    torch.cuda.synchronize()
    assert rc == OK, ("backward", rc)
    for k, b in g.items():
        assert b.margins_intact(), "written outside " + k
    for k in ("xt", "xdiag", "cls_out", "lse", "cls_lse", "dqkv"):         # NaN pre-fill: finite means written
        assert bool(torch.isfinite(g[k].data()).all()), "not fully written (or not finite): " + k
    for k, was in saved.items():                                          # the backward leaves what the forward saved alone
        assert torch.equal(g[k].data().view(was.dtype), was), "changed by the backward: " + k
    for k, src in (("qkv", qkv), ("dxt", cts[0]), ("dxdiag", cts[1]), ("dcls", cts[2])):
        assert torch.equal(g[k].data().cpu(), src.reshape(-1)), "input changed: " + k
    out = {"xt": g["xt"].data().view(B, S, F, C), "xd": g["xdiag"].data().view(B, S, C),
           "cls": g["cls_out"].data().view(B, 1, C), "dqkv": g["dqkv"].data().view(B, 1 + S, 3 * C)}
    return {k: v.cpu() for k, v in out.items()}, (nf, nb)


@pytest.mark.parametrize("case", sr.CASES, ids=[c[0] for c in sr.CASES])
def test_space_kernels_by_the_abi(case):
    _fused_or_skip()
    _, B, heads, F, P = case
    S, C = F * P, heads * sr.HD
    qkv, cts = sr.inputs(case)
    ref = sr.space_exact(qkv, F, P, heads, cts)
    got, (nf, nb) = run_abi(case, qkv, cts)
    # the route: the generic path's backward needs two S x S buffers and a copy of dxt on top of everything the fused one
    # needs.  (Below S = 64 the fixed paddings of the carve-up are larger than that; the rule itself is pinned without
    # a GPU in test_abi_cpu.py.)
    logits = B * heads * S * S * 2
    if S >= 64:
        assert nf < logits and nb < 2 * logits + B * S * F * C * 2, (nf, nb, logits)
    if S >= 512 and F <= 8:                                               # (F = 16: the lse / delta tables are S x 16 floats)
        assert 4 * nb < logits, (nb, logits)                              # far below one S x S logits buffer
    ck = Check()
    for what, g, w, mag, lim, floor in sr.quantities(got, ref):
        ck.tight(g, w, what, rtol=lim, floor=floor, mag=mag)
    ck.done()


def test_ops_layer_is_the_abi_call():
    """ops.traj_space + autograd give bit-identical outputs and gradients to the C-ABI call checked above."""
    _fused_or_skip()
    from focus_amd import ops
    case = ("ops_p33", 3, 3, 2, 33)
    qkv, cts = sr.inputs(case)
    got, _ = run_abi(case, qkv, cts)
    qg = qkv.to(dev()).requires_grad_()
    xt, xd, cls = ops.traj_space(qg, case[3], case[4], case[2])
    torch.autograd.backward([xt, xd, cls], [c.to(dev()) for c in cts])
    for k, t in (("xt", xt), ("xd", xd), ("cls", cls), ("dqkv", qg.grad)):
        assert t.dtype == BF16 and torch.equal(t.detach().cpu().view(torch.int16), got[k].view(torch.int16)), k
    ref = sr.space_exact(qkv, case[3], case[4], case[2], cts)
    ck = Check()
    for what, g, w, mag, lim, floor in sr.quantities(got, ref):
        ck.tight(g, w, what, rtol=lim, floor=floor, mag=mag)
    ck.done()


def test_more_frames_than_the_fused_kernels_hold():
    """F = 17: the lse table of the fused backward holds 16 frames, so the whole call -- workspace query, forward AND
    backward -- takes the generic path (it used to run the fused forward and refuse the backward).  Held to the generic
    bf16 route's figure of test_space_attention_key_tilings, not to rounding: the point is that both directions run."""
    case = ("f17_p3", 2, 2, 17, 3)
    _, B, heads, F, P = case
    S = F * P
    qkv, cts = sr.inputs(case)
    ref = sr.space_exact(qkv, F, P, heads, cts)
    got, (nf, nb) = run_abi(case, qkv, cts)
    logits = B * heads * S * S * 2
    assert nf >= logits and nb >= 2 * logits                              # the generic path's S x S buffers
    for k in ("xt", "xd", "cls", "dqkv"):
        err, top = float((got[k].double() - ref[k]).abs().max()), float(ref[k].abs().max())
        print("%-5s max|err| / max|ref| %.3e" % (k, err / top))
        assert err < 2.5e-2 * top, (k, err, top)


# Measured on an MI355X (FOCUS_MARGINS), largest |got - want| / max(|want|, mag) per row in units of U = 2^-8:
#
#   row         x~    x_diag  cls_out   dQ     dK     dV    token 0
#   limit      2.02    2.02    1.01    2.02   3.03   3.03    1.01
#   p1         0.00    0.00    0.98    0.00   0.67   1.61    0.98
#   p2         1.28    1.19    0.87    0.07   0.19   1.67    0.98
#   p31        1.04    0.94    0.97    0.12   0.23   1.73    0.96
#   p32_s128   0.98    0.86    0.94    0.09   0.12   1.12    0.93
#   p33        1.15    0.93    0.93    0.14   0.20   1.47    0.96
#   p64        0.95    0.95    0.92    0.15   0.18   1.52    0.96
#   p65        0.88    0.88    0.92    0.12   0.20   1.14    0.82
#   p96        0.94    0.88    0.96    0.11   0.12   0.98    0.98
#   p97_f5     0.90    0.89    0.98    0.06   0.08   1.03    0.95
#   p129       1.09    0.95    0.96    0.14   0.16   1.17    0.91
#   p160       0.92    0.92    0.98    0.13   0.10   0.67    0.77
#   p190       0.91    0.91    0.82    0.13   0.12   1.08    0.83
#   p196       0.88    0.86    0.96    0.15   0.16   1.53    0.97
#   p224       0.88    0.88    0.97    0.09   0.08   0.72    0.92
#   p225       0.95    0.91    0.90    0.16   0.10   1.36    0.84
#   p270       0.99    0.98    0.85    0.14   0.11   1.09    0.95
#   p288       1.05    1.04    0.85    0.14   0.13   1.28    0.94
#   p300       1.09    0.94    0.94    0.17   0.10   1.47    0.94
#   p330       1.07    1.07    0.86    0.24   0.11   1.09    0.91
#   p352       1.04    1.02    0.87    0.18   0.15   1.20    0.91
#   p353       1.04    0.94    0.94    0.15   0.16   1.38    0.93
#   p384       1.07    0.99    0.95    0.23   0.13   1.25    0.95
#   p390       1.10    1.01    0.95    0.16   0.10   0.99    0.87
#   p416       0.97    0.97    0.92    0.20   0.20   1.21    0.92
#   p417       0.95    0.94    0.88    0.17   0.15   1.87    0.92
#   p447       1.24    1.22    0.91    0.15   0.21   1.06    0.98
#   p448       1.12    1.12    0.90    0.17   0.17   1.17    0.95
#   f1_p20     0.91    0.91    0.92    0.22   0.31   1.90    0.97
#   f1_p40     0.85    0.85    0.94    0.18   0.22   1.42    0.97
#   f1_p70     0.96    0.96    0.96    0.15   0.20   1.47    0.96
#   s30        0.97    0.97    0.85    0.10   0.16   1.05    0.83
#   s50        0.99    0.94    0.97    0.17   0.21   1.28    0.96
#   s90        1.10    0.95    0.89    0.13   0.19   1.07    0.97
#   s129       0.92    0.86    0.89    0.12   0.15   1.14    0.94
#   f16_p5     1.45    1.44    0.94    0.06   0.08   0.92    0.99
#   f16_p33    1.16    0.97    0.81    0.04   0.05   0.38    0.87
#   ops_p33    1.12    0.93    0.95    0.16   0.24   1.34    0.97
#   max        1.45    1.44    0.98    0.24   0.67   1.90    0.99
#
# The rounding model of space_ref.py alone (no GPU) gives the same figure on every row (maxima 1.45 1.44 0.98 0.24 0.67
# 1.90 0.99): what is measured here is the kernels' own rounding points, nothing else.  Above half their limit: x~ / x_diag
# on most rows (1.0-1.45 U of 2.02: the output's rounding is near its worst case on some element of every row, the bf16
# probabilities add the rest; f16_p5 has 5 keys per frame, so little averages out); dV on p1, p2, p31, p64, p196, p417 and
# f1_p20 (1.5-1.9 U of 3.03: a key that one spiked query dominates carries that query's P rounding and both output
# roundings unaveraged); cls_out and the token-0 row are one output rounding, 0.8-0.99 U of 1.01 by construction.
# dQ and dK stay below 0.7 U.
# test_more_frames_than_the_fused_kernels_hold (generic route, limit 2.5e-2 of max|ref|): x~ 3.7e-3, x_diag 3.9e-3,
# cls 3.6e-3, dqkv 2.5e-3.
