"""Plain fp64 formulas of the slot tail (csrc/slot_tail.hip; STEVE/utils.py:107-118, steve.py:72-75, 85-93), stage by stage.
The checker of tests/test_gpu_slot_tail.py, itself checked without a GPU by tests/test_slot_tail_ref_cpu.py; the product
never imports this, and this imports neither a GPU nor focus_amd.

Every stage function takes the values a stage of the kernels READS (bf16 activations and weights, fp32 biases, LayerNorm
parameters and statistics; any float tensor, CPU or GPU) and returns fp64 values, the last of them `mag`: per output
element the sum of the absolute values of the terms it is formed from (sum_i |a_i b_i| + |bias| ...), the scale of the
classical error bound that Check.tight(..., mag=) expects.  Nothing is rounded in here; a caller that follows a kernel
which rounds between two stages rounds between the two calls.

Weights are [out, in] as the modules hold them (the backward kernels take the transposed copies; the formulas do not care).
  forward : gates, gru_gates, gru_out, ln, fc1_relu, fc2_res, q_proj
  backward: dsn, ln_bwd (dx and the per-block partials), dz, dy1, gate_bwd, dupd, dh
  tail    : the whole chain in fp64 without any rounding in between (differentiable: autograd gives its gradients)
  make_params / make_rows / make_grads: the seeded inputs of the GPU test; conditions(): what the CPU test asserts of them
"""
import torch

D, H, ROWS = 192, 768, 16
FLAGS = {"FFT": (0, 0, 1), "TFF": (1, 0, 0), "TFT": (1, 0, 1), "TTF": (1, 1, 0), "TTT": (1, 1, 1)}     # gru, mlp, q
R_ALL = (1, 15, 16, 17, 44, 352)
PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2", "ln2_g", "ln2_b", "wq")
EPS = 1e-5


def blocks(R):
    """focus_slot_tail_bwd_blocks(R)."""
    return (R + ROWS - 1) // ROWS


def _mm(x, w):
    """x [R, K] . w [N, K]^T -> (product, sum_k |x_k w_k|)."""
    x, w = x.double(), w.double()
    return x @ w.t(), x.abs() @ w.abs().t()


# ---- forward ------------------------------------------------------------------------------------------------------
def gates(upd, h, w_ih, w_hh, b_ih, b_hh):
    """-> gi, gh [R, 3D] (bias included), mag_i, mag_h."""
    gi, mi = _mm(upd, w_ih)
    gh, mh = _mm(h, w_hh)
    return gi + b_ih.double(), gh + b_hh.double(), mi + b_ih.double().abs(), mh + b_hh.double().abs()


def gru_gates(gi, gh):
    """-> r, z, n of torch.nn.GRUCell from its pre-activations (chunks r | z | n)."""
    gi, gh = gi.double(), gh.double()
    d = gi.shape[-1] // 3
    r = torch.sigmoid(gi[..., :d] + gh[..., :d])
    z = torch.sigmoid(gi[..., d:2 * d] + gh[..., d:2 * d])
    n = torch.tanh(gi[..., 2 * d:] + r * gh[..., 2 * d:])
    return r, z, n


def gru_out(gi, gh, h):
    """h' = (1 - z) n + z h -> hn, mag.  mag: the two terms, and what the argument of the tanh contributes through its
    slope, (1 - z)(1 - n^2)(|gi_n| + |r gh_n|) -- an fp32 error of r or of that sum reaches h' at this scale."""
    r, z, n = gru_gates(gi, gh)
    h = h.double()
    d = h.shape[-1]
    arg = gi.double()[..., 2 * d:].abs() + (r * gh.double()[..., 2 * d:]).abs()
    return (1 - z) * n + z * h, ((1 - z) * n).abs() + (z * h).abs() + (1 - z) * (1 - n * n) * arg


def ln(x, gamma, beta, eps=EPS):
    """-> y, mean, rstd (biased variance), mag, mean|x| per row.  mag = |gamma| rstd (|x| + mean|x|) + |beta|: the terms of
    (x - mean) rstd gamma + beta, with mean|x| >= |mean| because the error of a computed mean is relative to mean|x|."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    mabs = x.abs().mean(-1, keepdim=True)
    y = (x - mean) * rstd * gamma + beta
    return y, mean[..., 0], rstd[..., 0], gamma.abs() * rstd * (x.abs() + mabs) + beta.abs(), mabs[..., 0]


def fc1_relu(y, w1, b1):
    v, m = _mm(y, w1)
    return torch.relu(v + b1.double()), m + b1.double().abs()


def fc2_res(a, w2, b2, hn):
    v, m = _mm(a, w2)
    return v + b2.double() + hn.double(), m + b2.double().abs() + hn.double().abs()


def q_proj(sn, wq):
    return _mm(sn, wq)


# ---- backward -----------------------------------------------------------------------------------------------------
def _mm_t(dy, w):
    """dy [R, N] . w [N, K] -> (product [R, K], sum_n |dy_n w_n|)."""
    dy, w = dy.double(), w.double()
    return dy @ w, dy.abs() @ w.abs()


def dsn(dq, wq):
    return _mm_t(dq, wq)


def ln_bwd(dy, x, gamma, mean, rstd, res=None, dy_mag=None):
    """LayerNorm backward on the statistics the forward stored: xhat = (x - mean) rstd,
        dx = rstd (dy g - mean_c(dy g) - xhat mean_c(dy g xhat)) [+ res]
        part[0][blk][c] = sum over the rows of 16-row block blk of dy xhat,  part[1][blk][c] = the same of dy
    -> dx [R, D], part [2, blocks(R), D], mag_dx, mag_part.  dy_mag (optional, >= |dy|): the magnitude of the product dy
    was rounded from, where the caller had to round it itself; it replaces |dy| in mag_dx and mag_part."""
    dy, x, gamma = dy.double(), x.double(), gamma.double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    xh = (x - mean) * rstd
    dg = dy * gamma
    dx = rstd * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
    ady = dy.abs() if dy_mag is None else torch.maximum(dy.abs(), dy_mag.double())
    adg = ady * gamma.abs()
    mag = rstd * (adg + adg.mean(-1, keepdim=True) + xh.abs() * (adg * xh.abs()).mean(-1, keepdim=True))
    if res is not None:
        dx, mag = dx + res.double(), mag + res.double().abs()
    R, d = dy.shape
    nb = blocks(R)
    blk = (torch.arange(R, device=dy.device) // ROWS)[:, None].expand(R, d)
    part = dy.new_zeros(2, nb, d)
    mpart = dy.new_zeros(2, nb, d)
    part[0].scatter_add_(0, blk, dy * xh)
    part[1].scatter_add_(0, blk, dy)
    mpart[0].scatter_add_(0, blk, ady * xh.abs())             # (x and the stored mean are exact inputs: x - mean rounds once)
    mpart[1].scatter_add_(0, blk, ady)
    return dx, part, mag, mpart


def dz(ds, w2, a):
    """(ds W2) * (a > 0); w2 [D, H]."""
    v, m = _mm_t(ds, w2)
    return v * (a.double() > 0), m


def dy1(dz_, w1):
    """dz W1; w1 [H, D]."""
    return _mm_t(dz_, w1)


def gate_bwd(gi, gh, h, dhn, dhn_mag=None):
    """The GRU cell's backward from its stored pre-activations: with r, z, n as in gru_gates and d = dhn,
        dn_pre = d (1 - z)(1 - n^2);  dgi = [dn_pre gh_n r (1 - r) | d (h - n) z (1 - z) | dn_pre];  dgh = the same with
        dn_pre r as its third chunk;  res = d z (the direct path into dh).
    -> dgi, dgh [R, 3D], res [R, D], mag_gi, mag_gh, mag_res.  The magnitudes hold |d| (or dhn_mag >= |d|), |h| + |n| for
    h - n and 1 + n^2 for 1 - n^2: the places where fp32 terms cancel."""
    r, z, n = gru_gates(gi, gh)
    h, d_ = h.double(), dhn.double()
    d = h.shape[-1]
    ghn = gh.double()[..., 2 * d:]
    ad = d_.abs() if dhn_mag is None else torch.maximum(d_.abs(), dhn_mag.double())
    dn_pre = d_ * (1 - z) * (1 - n * n)
    m_pre = ad * (1 - z) * (1 + n * n)
    pr, m_r = dn_pre * ghn * r * (1 - r), m_pre * ghn.abs() * r * (1 - r)
    pz, m_z = d_ * (h - n) * z * (1 - z), ad * (h.abs() + n.abs()) * z * (1 - z)
    dgi = torch.cat([pr, pz, dn_pre], -1)
    dgh = torch.cat([pr, pz, dn_pre * r], -1)
    return dgi, dgh, d_ * z, torch.cat([m_r, m_z, m_pre], -1), torch.cat([m_r, m_z, m_pre * r], -1), ad * z


def dupd(dgi, w_ih):
    return _mm_t(dgi, w_ih)


def dh(dgh, w_hh, res):
    v, m = _mm_t(dgh, w_hh)
    return v + res.double(), m + res.double().abs()


# ---- the whole chain ----------------------------------------------------------------------------------------------
def tail(upd, h, p, flags, eps=EPS):
    """-> (slots, q or None) in fp64 with nothing rounded in between; p: dict over PARAMS.  Differentiable."""
    gru, mlp, q = flags
    assert gru or not mlp
    P = {k: v.double() for k, v in p.items()}
    cur = h.double()
    if gru:
        gi, gh, _, _ = gates(upd, cur, P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"])
        cur = gru_out(gi, gh, cur)[0]
    if mlp:
        y = ln(cur, P["ln1_g"], P["ln1_b"], eps)[0]
        a = fc1_relu(y, P["w1"], P["b1"])[0]
        cur = fc2_res(a, P["w2"], P["b2"], cur)[0]
    qv = None
    if q:
        qv = q_proj(ln(cur, P["ln2_g"], P["ln2_b"], eps)[0], P["wq"])[0]
    return cur, qv


# ---- the inputs of the GPU test -------------------------------------------------------------------------------------
def make_params(seed=7):
    """GRU and Linear weights uniform in +-fan_in^-1/2 like the modules' initialisation, rounded to bf16 (the kernels take
    the bf16 working copies); fp32 biases of the same range, LayerNorm gains 1 + 0.1 N(0,1), nonzero LayerNorm shifts."""
    g = torch.Generator().manual_seed(seed)
    uni = lambda *s, fan: (torch.rand(*s, generator=g) * 2 - 1) * fan ** -0.5
    p = {"w_ih": uni(3 * D, D, fan=D).bfloat16(), "w_hh": uni(3 * D, D, fan=D).bfloat16(),
         "b_ih": uni(3 * D, fan=D), "b_hh": uni(3 * D, fan=D),
         "ln1_g": 1 + 0.1 * torch.randn(D, generator=g), "ln1_b": 0.1 * torch.randn(D, generator=g) + 0.05,
         "w1": uni(H, D, fan=D).bfloat16(), "b1": uni(H, fan=D),
         "w2": uni(D, H, fan=H).bfloat16(), "b2": uni(D, fan=H),
         "ln2_g": 1 + 0.1 * torch.randn(D, generator=g), "ln2_b": 0.1 * torch.randn(D, generator=g) - 0.05,
         "wq": uni(D, D, fan=D).bfloat16()}
    assert tuple(p) == PARAMS
    return p


def make_rows(R, seed=100):
    """upd, h: N(0,1) rounded to bf16."""
    g = torch.Generator().manual_seed(seed + R)
    return torch.randn(R, D, generator=g).bfloat16(), torch.randn(R, D, generator=g).bfloat16()


def make_grads(R, seed=200):
    """dout, dq: N(0,1) rounded to bf16."""
    g = torch.Generator().manual_seed(seed + R)
    return torch.randn(R, D, generator=g).bfloat16(), torch.randn(R, D, generator=g).bfloat16()


def conditions(R, p=None):
    """What makes the inputs of one R a test: -> dict(zero_a: share of a == 0, open_gates: share of r and z inside
    (0.02, 0.98), min_var: smallest variance of a row any LayerNorm of any flag combination normalises)."""
    p = make_params() if p is None else p
    P = {k: v.double() for k, v in p.items()}
    upd, h = make_rows(R)
    gi, gh, _, _ = gates(upd, h, P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"])
    r, z, _ = gru_gates(gi, gh)
    hn = gru_out(gi, gh, h)[0]
    a = fc1_relu(ln(hn, P["ln1_g"], P["ln1_b"])[0], P["w1"], P["b1"])[0]
    s = fc2_res(a, P["w2"], P["b2"], hn)[0]
    rz = torch.cat([r, z], -1)
    return {"zero_a": float((a == 0).double().mean()),
            "open_gates": float(((rz > 0.02) & (rz < 0.98)).double().mean()),
            "min_var": min(float(t.double().var(-1, unbiased=False).min()) for t in (h, hn, s))}
