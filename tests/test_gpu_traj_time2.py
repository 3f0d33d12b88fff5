"""The k2-free temporal attention kernels (csrc/traj_time2.hip, csrc/traj_time2_gw.hip) by the C ABI against
tests/time_ref.py in fp64: all 25 kernel instances the dispatch reaches by default (frame counts 4, 8, 16; 1 to 4 weight
units per wave; staged and direct), row counts from 1 to 1281 chosen against the tile, the owner ranges and the ring turns,
B = 1 and B = 3 with tiles that straddle a batch boundary, every weight pitch and batch stride -- and, in child processes,
the 17 direct instances of FOCUS_T2_LDS=0 and the second owner table of FOCUS_T2_SPREAD=1.  Which instance a row reaches
is not observable from outside: time_ref.route restates the dispatch and test_time_ref_cpu.py checks it and the table.

Every buffer lives inside a larger one with a margin in front and behind; outputs, margins, the workspace, the unused
columns of a wide weight matrix and the gap of a wide batch stride are pre-filled with NaN bit patterns no kernel produces,
and the workspace is exactly focus_traj_time2_workspace_bytes long.  After forward and backward every margin is
bit-identical, every output element is finite (so: written), inputs and the saved attn2 are unchanged, the padded columns
of dl are +0, and every element of every quantity is held to the counted limits of time_ref.py: each kernel against its
stage reference fed the DEVICE's upstream tensors, and out, g, dx~ end to end against the original form.

With FOCUS_MARGINS set every test appends its largest error over magnitude per quantity; the figures measured on an MI355X
are the comment at the end of this file."""
import os
import subprocess
import sys
import time

import pytest
import torch

import time_ref as tr
from test_gpu_kernels import Check
from test_gpu_parity import dev
from test_gpu_traj_space import BF16, F32, FILL, OK, U8, Guarded, _stream

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ALIGN, ERR_NULL, ERR_WORKSPACE = -1, -3, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TABLE_SECONDS = {}                                               # measured time of the in-process table, per row


def _time2_or_skip():
    if os.environ.get("FOCUS_TIME2", "1").strip() == "0":
        pytest.skip("FOCUS_TIME2=0: the k2-free temporal kernels are switched off in this environment")


def _nan_filled(shape, dtype):
    it, fill = FILL[dtype]
    return torch.full(shape, fill, dtype=it).view(dtype)


def _bits(t):
    return t.view(FILL[t.dtype][0])


def _hold(ck, rows):
    for what, got, want, mag, lim in rows:
        err = got.double() - want
        ck.tight(err, torch.zeros_like(err), what, rtol=lim, floor=0.0, mag=mag)


class Time2Call:
    """The guarded buffers of one row of time_ref.CASES and the two ABI calls on them."""

    def __init__(self, case, tensors):
        from focus_amd import _lib
        self.L, self.case = _lib.lib(), case
        _, B, S, F, heads = case[:5]
        C, R = heads * tr.HD, B * S
        self.ldw, self.bs = tr.ldw_of(case), tr.bstride_of(case)
        self.dims = (B, S, F, heads, tr.HD, _lib.BF16)
        q2, xt, wk, _, _, ct = tensors
        wkT = _nan_filled((C, self.ldw), BF16)                    # columns C.. are never read: NaN
        wkT[:, :C] = wk.t()
        self.span = (B - 1) * self.bs + (S + 1) * C               # the [B, 1+S, C] window at batch stride bs
        dout = _nan_filled((self.span,), BF16)                    # the gap of a wide stride is never read: NaN
        for b in range(B):
            dout[b * self.bs:b * self.bs + (S + 1) * C] = ct[b].reshape(-1)
        self.src = {"q2": q2.reshape(-1), "xt": xt.reshape(-1), "wkT": wkT.reshape(-1), "dout": dout}
        self.g = {k: Guarded(v.numel(), BF16, v.to(dev())) for k, v in self.src.items()}
        self.nws = self.L.focus_traj_time2_workspace_bytes(*self.dims[:5])
        assert self.nws == heads * R * heads * F * 4
        self.g.update({"out": Guarded(self.span, BF16), "attn2": Guarded(R * heads * F, F32), "ws": Guarded(self.nws, U8),
                       "dxt": Guarded(R * F * C, BF16), "g": Guarded(heads * R * C, BF16), "dl": Guarded(R * F * tr.MAXH, BF16)})
        self.C, self.R = C, R

    def rows_ptr(self, k):
        """out / dout: the rows start one row (the cls row) into the window"""
        return self.g[k].ptr() + self.C * 2

    def fwd(self, **over):
        a = dict(q2=self.g["q2"].ptr(), xt=self.g["xt"].ptr(), wkT=self.g["wkT"].ptr(), ldw=self.ldw, out=self.rows_ptr("out"),
                 bs=self.bs, attn2=self.g["attn2"].ptr(), ws=self.g["ws"].ptr(), nws=self.nws, dims=self.dims)
        a.update(over)
        rc = self.L.focus_traj_time2_fwd(a["q2"], a["xt"], a["wkT"], a["ldw"], a["out"], a["bs"], a["attn2"], a["ws"], a["nws"],
                                         *a["dims"], _stream())
        torch.cuda.synchronize()
        return rc

    def bwd(self, **over):
        a = dict(q2=self.g["q2"].ptr(), xt=self.g["xt"].ptr(), wkT=self.g["wkT"].ptr(), ldw=self.ldw, attn2=self.g["attn2"].ptr(),
                 dout=self.rows_ptr("dout"), bs=self.bs, dxt=self.g["dxt"].ptr(), g=self.g["g"].ptr(), dl=self.g["dl"].ptr(),
                 dims=self.dims)
        a.update(over)
        rc = self.L.focus_traj_time2_bwd(a["q2"], a["xt"], a["wkT"], a["ldw"], a["attn2"], a["dout"], a["bs"], a["dxt"], a["g"],
                                         a["dl"], *a["dims"], _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self, keys):
        """every element of these buffers still holds its pre-fill bits"""
        return [k for k in keys if not bool((self.g[k].buf == self.g[k].fill).all())]

    def window(self, k):
        """out / dout as a [B, 1+S, C] copy (the gaps of a wide batch stride left out)"""
        _, B, S = self.case[:3]
        d = self.g[k].data()
        return torch.stack([d[b * self.bs:b * self.bs + (S + 1) * self.C].view(S + 1, self.C) for b in range(B)])

    def run(self):
        """Forward and backward with every structural assertion.  -> (flat outputs on the device, their bits)."""
        _, B, S, F, heads = self.case[:5]
        C, R = self.C, self.R
        assert self.fwd() == OK
        att_saved = _bits(self.g["attn2"].data()).clone()
        out_saved = _bits(self.g["out"].data()).clone()
        assert self.untouched(("dxt", "g", "dl")) == []
        assert self.bwd() == OK
        for k, b in self.g.items():
            assert b.margins_intact(), "written outside " + k
        for k, v in self.src.items():
            assert torch.equal(_bits(self.g[k].data()).cpu(), _bits(v)), "input changed: " + k
        assert torch.equal(_bits(self.g["attn2"].data()), att_saved), "attn2 changed by the backward"
        assert torch.equal(_bits(self.g["out"].data()), out_saved), "out changed by the backward"
        ow = self.window("out")
        for k, t in (("out", ow[:, 1:]), ("attn2", self.g["attn2"].data()), ("dxt", self.g["dxt"].data()),
                     ("g", self.g["g"].data()), ("dl", self.g["dl"].data())):
            assert bool(torch.isfinite(t).all()), "not fully written (or not finite): " + k
        fill = FILL[BF16][1]
        assert bool((_bits(ow[:, 0]) == fill).all()), "the cls row of out was written"
        keep = torch.ones(self.span, dtype=torch.bool, device=dev())
        for b in range(B):
            keep[b * self.bs:b * self.bs + (S + 1) * C] = False
        assert bool((_bits(self.g["out"].data())[keep] == fill).all()), "the gap of the batch stride was written"
        dl16 = self.g["dl"].data().view(R, F, tr.MAXH)
        assert bool((_bits(dl16)[:, :, heads:] == 0).all()), "dl columns heads..15 are not +0"
        res = {"attn": self.g["attn2"].data().view(R, heads, F), "out": ow[:, 1:].reshape(R, C),
               "dl": dl16[:, :, :heads].transpose(1, 2), "g": self.g["g"].data().view(heads, R, C),
               "dxt": self.g["dxt"].data().view(R, F, C)}
        bits = {k: _bits(self.g[k].data()).clone() for k in ("out", "attn2", "dxt", "g", "dl")}
        return res, bits


def _on_dev(tensors):
    return tuple(t.to(dev()) for t in tensors)


@pytest.mark.parametrize("case", tr.CASES, ids=[c[0] for c in tr.CASES])
def test_time2_by_the_abi(case):
    _time2_or_skip()
    t0 = time.perf_counter()
    heads = case[4]
    tensors = tr.inputs(case)
    got, bits = Time2Call(case, tensors).run()
    q2, xt, wk, bk, cls, ct = _on_dev(tensors)                    # the fp64 reference is computed on the device
    ex = tr.time_exact(q2, xt, wk, bk, cls, ct, heads)
    ck = Check()
    _hold(ck, tr.quantities(tr.flat(case, q2, xt, wk, ct), got, ex))
    again, bits2 = Time2Call(case, tensors).run()                 # fresh buffers, fresh pre-fill
    for k in bits:
        assert torch.equal(bits[k], bits2[k]), "a second launch gives other bits: " + k
    ck.done()
    _TABLE_SECONDS[case[0]] = time.perf_counter() - t0


class GwCall:
    """The guarded buffers of one row of time_ref.GW_CASES (or of a device g) and the ABI call on them."""

    def __init__(self, R, wk_ld, g_, q2, wk):
        from focus_amd import _lib
        self.L = _lib.lib()
        C = tr.GW_C
        wkp = _nan_filled((C, wk_ld), BF16)
        wkp[:, :C] = wk.cpu()
        self.src = {"g": g_.reshape(-1), "q2": q2.reshape(-1), "wk": wkp.reshape(-1)}
        self.g = {k: Guarded(v.numel(), BF16, v.to(dev())) for k, v in self.src.items()}
        self.nws = self.L.focus_traj_time2_gw_workspace_bytes(R, tr.GW_HEADS, tr.HD)
        assert self.nws == tr.gw_route(R)["splits"] * C * C * 4
        self.g.update({"dq2": Guarded(R * C, BF16), "dwk": Guarded(C * C, F32), "ws": Guarded(self.nws, U8)})
        self.R, self.wk_ld, self.dims = R, wk_ld, (R, tr.GW_HEADS, tr.HD, _lib.BF16)

    def call(self, **over):
        a = dict(g=self.g["g"].ptr(), q2=self.g["q2"].ptr(), wk=self.g["wk"].ptr(), wk_ld=self.wk_ld, dq2=self.g["dq2"].ptr(),
                 dwk=self.g["dwk"].ptr(), ws=self.g["ws"].ptr(), nws=self.nws, dims=self.dims)
        a.update(over)
        rc = self.L.focus_traj_time2_gw(a["g"], a["q2"], a["wk"], a["wk_ld"], a["dq2"], a["dwk"], a["ws"], a["nws"], *a["dims"],
                                        _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self, keys):
        return [k for k in keys if not bool((self.g[k].buf == self.g[k].fill).all())]

    def run(self):
        assert self.call() == OK
        for k, b in self.g.items():
            assert b.margins_intact(), "written outside " + k
        for k, v in self.src.items():
            assert torch.equal(_bits(self.g[k].data()).cpu(), _bits(v.cpu())), "input changed: " + k
        for k in ("dq2", "dwk"):
            assert bool(torch.isfinite(self.g[k].data()).all()), "not fully written (or not finite): " + k
        return {"dq2": self.g["dq2"].data().view(self.R, tr.GW_C), "dwk": self.g["dwk"].data().view(tr.GW_C, tr.GW_C)}


@pytest.mark.parametrize("case", tr.GW_CASES, ids=[c[0] for c in tr.GW_CASES])
def test_time2_gw_by_the_abi(case):
    _, R, wk_ld = case
    g_, q2, wk = tr.gw_inputs(case)
    got = GwCall(R, wk_ld, g_, q2, wk).run()
    ck = Check()
    _hold(ck, tr.gw_quantities(g_.to(dev()), q2.to(dev()), wk.to(dev()), got))
    again = GwCall(R, wk_ld, g_, q2, wk).run()
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(again[k])), "a second launch gives other bits: " + k
    ck.done()


def test_time2_status_codes_leave_outputs_alone():
    """Every refused call returns the code include/focus_amd.h documents and writes nothing."""
    _time2_or_skip()
    case = ("status", 2, 5, 4, 2, "C+8", 8, "unit")
    _, B, S, F, heads = case[:5]
    C = heads * tr.HD
    tensors = tr.inputs(case)
    t = Time2Call(case, tensors)
    outs = ("out", "attn2", "ws", "dxt", "g", "dl")
    dims = lambda **kw: tuple(kw.get(k, v) for k, v in zip(("B", "S", "F", "heads", "d", "dtype"), t.dims))
    shape_errors = [dict(dims=dims(F=5)), dict(dims=dims(heads=17)), dict(dims=dims(heads=0)), dict(dims=dims(d=32)),
                    dict(dims=dims(dtype=0)), dict(ldw=C - 8), dict(ldw=C + 4), dict(bs=S * C - 8), dict(bs=(S + 1) * C + 4),
                    dict(dims=dims(B=0)), dict(dims=dims(S=0))]
    for name, call, ptrs in (("fwd", t.fwd, ("q2", "xt", "wkT", "out", "attn2", "ws")),
                             ("bwd", t.bwd, ("q2", "xt", "wkT", "attn2", "dout", "dxt", "g", "dl"))):
        for p in ptrs:
            assert call(**{p: None}) == ERR_NULL, (name, p)
        for kw in shape_errors:
            assert call(**kw) == ERR_SHAPE, (name, kw)
        for p in ptrs:
            if name == "bwd" and p == "attn2":                   # fp32, read 4 bytes at a time: not judged
                continue
            base = t.rows_ptr(p) if p in ("out", "dout") else t.g[p].ptr()
            assert call(**{p: base + 2}) == ERR_ALIGN, (name, p)
        assert t.untouched(outs) == [], name
    assert t.fwd(nws=t.nws - 1) == ERR_WORKSPACE
    assert t.fwd(ldw=C - 8, nws=0) == ERR_SHAPE                   # the order: shape before workspace
    assert t.fwd(q2=None, dims=dims(F=5)) == ERR_NULL             # ... and null before shape
    assert t.untouched(outs) == []
    assert t.L.focus_traj_time2_workspace_bytes(0, S, F, heads, 64) == 0
    assert t.L.focus_traj_time2_workspace_bytes(B, S, F, heads, 32) == 0
    t.run()                                                       # the same buffers still serve a good call

    R = 64
    g_, q2, wk = tr.gw_inputs(("status_gw", R, 776))
    w = GwCall(R, 776, g_, q2, wk)
    gouts = ("dq2", "dwk", "ws")
    for p in ("g", "q2", "wk", "dq2", "dwk", "ws"):
        assert w.call(**{p: None}) == ERR_NULL, p
    for kw in (dict(dims=(48, 12, 64, 1)), dict(dims=(0, 12, 64, 1)), dict(dims=(R, 6, 64, 1)), dict(dims=(R, 12, 32, 1)),
               dict(dims=(R, 12, 64, 0)), dict(wk_ld=772)):
        assert w.call(**kw) == ERR_SHAPE, kw
    for p in ("g", "q2", "wk", "dwk"):
        assert w.call(**{p: w.g[p].ptr() + 2}) == ERR_ALIGN, p
    assert w.call(nws=w.nws - 1) == ERR_WORKSPACE
    assert w.untouched(gouts) == []
    assert w.L.focus_traj_time2_gw_workspace_bytes(48, 12, 64) == 0 and not w.L.focus_traj_time2_gw_ok(R, 6, 64, 1)
    w.run()


@pytest.mark.parametrize("case", [("ops_gw", 2, 48, 4, 12, "2C", 0, "unit"), ("ops_gemm", 1, 21, 8, 3, "2C", 0, "unit")],
                         ids=["gw", "two_gemms"])
def test_ops_layer_is_the_abi_call(case):
    """ops.traj_time2_block + autograd give bit-identical out, dx~ (and, where focus_traj_time2_gw takes the row, dq2 and
    dWk) to the C-ABI calls checked above; the two batched GEMMs of the other rows are held to the same limits."""
    _time2_or_skip()
    from focus_amd import ops
    _, B, S, F, heads = case[:5]
    C, R = heads * tr.HD, B * S
    tensors = tr.inputs(case)
    got, _ = Time2Call(case, tensors).run()
    q2, xt, wk, bk, cls, ct = _on_dev(tensors)
    qg, xg, cg = (t.clone().requires_grad_() for t in (q2, xt, cls))
    w_kv = torch.cat([wk, wk.flip(0)], 0).float().requires_grad_()           # fp32 parameter holding bf16 values
    b_kv = torch.zeros(2 * C, device=dev()).requires_grad_()
    assert ops.traj_time2_ok(xt, heads)
    y = ops.traj_time2_block(qg, xg, w_kv, b_kv, cg, heads)
    y.backward(ct)
    same = lambda a, b: a.dtype == b.dtype and torch.equal(_bits(a.detach().contiguous()), _bits(b.contiguous()))
    assert same(y[:, 1:].reshape(R, C), got["out"]) and same(y[:, :1], cls)
    assert same(xg.grad.reshape(R, F, C), got["dxt"])
    assert same(cg.grad, ct[:, :1]) and float(b_kv.grad.abs().max()) == 0.0 and float(w_kv.grad[C:].abs().max()) == 0.0
    from focus_amd import _lib
    L = _lib.lib()
    gw =bool(L.focus_traj_time2_gw_ok(R, heads, tr.HD, 1)) and os.environ.get("FOCUS_TIME2_GW", "1") != "0"
    assert bool(L.focus_traj_time2_gw_ok(R, heads, tr.HD, 1)) == (case[0] == "ops_gw")
    mine = {"dq2": qg.grad.reshape(R, C), "dwk": w_kv.grad[:C]}
    if gw:
        abi = GwCall(R, C, got["g"].cpu(), q2.cpu(), wk).run()
        assert same(mine["dq2"], abi["dq2"]) and same(mine["dwk"], abi["dwk"])
    ck = Check()
    _hold(ck, tr.gw_quantities(got["g"], q2.reshape(R, C), wk, mine))
    ck.done()


def test_time2_switched_kernels_in_a_child_process():
    """FOCUS_T2_LDS and FOCUS_T2_SPREAD are read once per process: the direct instances the staged ones shadow and the second
    owner table are reached in a fresh process only.  Runs test_time2_by_the_abi there, one child at a time."""
    _time2_or_skip()
    measured = sum(_TABLE_SECONDS.values()) if len(_TABLE_SECONDS) == len(tr.CASES) else 60.0
    limit = 3.0 * measured + 120.0                                # the table again, plus interpreter and runtime start-up
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "test_time2_by_the_abi"]
    for switch in ("FOCUS_T2_LDS=0", "FOCUS_T2_SPREAD=1"):
        env = {k: v for k, v in os.environ.items() if k not in ("FOCUS_T2_LDS", "FOCUS_T2_SPREAD", "FOCUS_MARGINS")}
        env[switch.split("=")[0]] = switch.split("=")[1]
        if os.environ.get("FOCUS_MARGINS"):
            env["FOCUS_MARGINS"] = os.environ["FOCUS_MARGINS"] + "." + switch
        try:
            p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired as e:
            pytest.fail("%s: the child ran into its limit of %.0f s; no further child is started\n%s"
                        % (switch, limit, (e.stdout or b"")[-2000:]), pytrace=False)
        tail = (p.stdout + p.stderr)[-3000:]
        if p.returncode < 0:
            pytest.fail("%s: the child ended by signal %d; no further child is started\n%s" % (switch, -p.returncode, tail),
                        pytrace=False)
        assert p.returncode == 0, "%s: the table fails in the child\n%s" % (switch, tail)
        assert "%d passed" % len(tr.CASES) in p.stdout, (switch, tail)


# Measured on an MI355X (FOCUS_MARGINS), largest |got - want| / magnitude per row as a fraction of its limit (stage rows:
# the reference is fed the device's own upstream tensors; "vs exact": end to end against the original form):
#
#   row            attn2   out    dl     g     dx~  | out    g     dx~ vs exact |  dq2   dWk
#   f4_h1_r1        0.02  0.68  0.25  0.29  0.54   0.07  0.02  0.07
#   f4_h3_r15       0.07  0.92  0.63  0.61  0.72   0.07  0.04  0.07
#   f4_h5_r17       0.08  0.92  0.79  0.65  0.73   0.05  0.03  0.07
#   f4_h9_s37       0.06  0.97  0.91  0.81  0.68   0.05  0.03  0.04
#   f4_h13_s21      0.05  0.98  0.93  0.75  0.64   0.04  0.02  0.02
#   f4_h16_s50      0.05  0.97  0.94  0.77  0.93   0.04  0.03  0.02
#   f8_h1_r16       0.13  0.81  0.70  0.44  0.79   0.09  0.04  0.17
#   f8_h1_s35       0.17  0.92  0.82  0.55  0.86   0.10  0.05  0.17
#   f8_h4_s19       0.09  0.94  0.84  0.56  0.80   0.06  0.03  0.07
#   f8_h8_s43       0.05  0.95  0.90  0.63  0.80   0.05  0.02  0.04
#   f8_h11_s29      0.07  0.97  0.94  0.85  0.94   0.03  0.03  0.03
#   f8_h12_r1280    0.06  0.97  0.94  0.70  0.73   0.04  0.03  0.04
#   f8_h12_r1281    0.08  0.98  0.98  0.82  0.88   0.04  0.05  0.05
#   f8_h13_s23      0.05  0.97  0.86  0.64  0.68   0.03  0.02  0.02
#   f8_h14_s18      0.04  0.93  0.84  0.65  0.61   0.04  0.02  0.02
#   f8_h15_s33      0.04  0.96  0.88  0.66  0.68   0.03  0.02  0.03
#   f8_h16_s300     0.05  0.97  0.90  0.70  0.68   0.03  0.03  0.03
#   f16_h3_s21      0.11  0.87  0.78  0.48  0.80   0.05  0.02  0.08
#   f16_h5_r15      0.07  0.81  0.78  0.53  0.76   0.04  0.02  0.05
#   f16_h8_s27      0.07  0.95  0.98  0.65  0.84   0.04  0.02  0.06
#   f16_h9_s33      0.06  0.90  0.79  0.51  0.72   0.04  0.02  0.05
#   f16_h12_s45     0.05  0.83  0.84  0.56  0.78   0.03  0.02  0.04
#   f16_h16_s21     0.04  0.86  0.88  0.55  0.70   0.03  0.02  0.03
#   gw_r32 .. gw_r1376 (six rows)                                                  0.97-0.98  0.02-0.05
#   ops gw / two_gemms                                                             0.98 0.97  0.04 0.05
#   max             0.17  0.98  0.98  0.85  0.94   0.10  0.05  0.17                 0.98  0.05
#
# The children under FOCUS_T2_LDS=0 and under FOCUS_T2_SPREAD=1 give the same figure in every cell of the table (the direct
# and the staged kernels issue the same MFMAs in the same order; the owner table only moves tiles between workgroups).
# The rounding model of time_ref.py alone (no GPU) has the maxima 0.17 0.98 0.98 0.86 0.94 | 0.10 0.05 0.18 | 0.98 0.00:
# what is measured here is the kernels' own rounding points, nothing else (dWk: the model is exact, the kernel's fp32
# chains use 2-5 % of FP32_CHAIN).  Near their limit by construction: out, dl and dq2 are ONE bf16 rounding each, which
# comes close to its worst case U on some element of every row with a few thousand elements; g is one rounding against
# the uncancelled sum_f mag_dl |x~|; dx~ (two roundings) reaches 0.94 where sum_h |dl||u| dominates a|dout| (the +-60 rows
# f4_h16_s50, f8_h11_s29).  attn2 and the end-to-end rows stay below 0.2: their magnitudes are worst-case first-order
# bounds over 64..1024 channels whose rounding errors do not align.
