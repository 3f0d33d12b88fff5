"""Greedy generation with cached keys and values on the GPU: focus_decode_attn and focus_greedy_next (csrc/decode_attn.hip)
against fp64, TransformerDecoder.step against the oracle's full pass, and STEVE.decode's cached token loop against the
incremental fp64 reference of tests/decode_ref.py, the loop it replaces, and the route it takes."""
import zlib

import pytest
import torch

import attn_ref
import decode_ref
from test_gpu_parity import close, dev

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
LMAX = 1024
LENS = (1, 2, 63, 64, 65, 255, 256, 257, 1024)          # around the kernel's key-loop boundaries, first and last row
GUARD = 2


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _one_decode_call(B, heads, d, length, lmax, append, packed, dtype, tag):
    """One focus_decode_attn call on seeded inputs -> (err of the output against fp64 on the storage-rounded inputs, and
    the in-place checks as a list of failure strings)."""
    from focus_amd import ops
    dv = dev()
    C = heads * d
    g = torch.Generator().manual_seed(zlib.crc32(("%s-%d-%d-%d-%d" % (tag, B, heads, d, length)).encode()))
    rnd = lambda *s: torch.randn(*s, generator=g)
    qkv = torch.cat([rnd(B, C) * 0.7, rnd(B, C) * 0.7, rnd(B, C)], dim=1).to(dtype)
    # caches with GUARD rows before and after each clip's lmax rows; rows >= the valid prefix hold NaN
    kbuf, vbuf = (rnd(B, lmax + 2 * GUARD, C) * 0.7).to(dtype), rnd(B, lmax + 2 * GUARD, C).to(dtype)
    old = length - 1 if append else length
    kbuf[:, GUARD + old:GUARD + lmax] = float("nan")
    vbuf[:, GUARD + old:GUARD + lmax] = float("nan")
    kexp, vexp = kbuf.clone(), vbuf.clone()
    if append:
        kexp[:, GUARD + length - 1] = qkv[:, C:2 * C]
        vexp[:, GUARD + length - 1] = qkv[:, 2 * C:]
    scale = d ** -0.5
    exact = decode_ref.decode_attention(qkv[:, :C], kexp[:, GUARD:GUARD + lmax], vexp[:, GUARD:GUARD + lmax], length, heads,
                                        scale)
    qg, kg, vg = qkv.to(dv), kbuf.to(dv), vbuf.to(dv)
    if packed:                                            # the column blocks of one [B, 3C] projection output
        q, kn, vn = qg[:, :C], qg[:, C:2 * C], qg[:, 2 * C:]
    else:
        q, kn, vn = (qg[:, i * C:(i + 1) * C].contiguous() for i in range(3))
    out = ops.decode_attention(q, kn if append else None, vn if append else None, kg[:, GUARD:GUARD + lmax],
                               vg[:, GUARD:GUARD + lmax], length, heads, scale)
    bad = []
    if out.shape != (B, C) or out.dtype != dtype:
        bad.append("output shape / dtype")
    if not bool(torch.isfinite(out.float()).all()):
        bad.append("non-finite output")
    # row length-1 is k_new / v_new bit for bit, everything else (guard rows included) is what it was
    if not torch.equal(_bits(kg.cpu()), _bits(kexp)):
        bad.append("k cache bits")
    if not torch.equal(_bits(vg.cpu()), _bits(vexp)):
        bad.append("v cache bits")
    if not torch.equal(_bits(qg.cpu()), _bits(qkv)):
        bad.append("inputs written")
    return attn_ref.err(out.cpu(), exact), bad


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("heads,d", [(2, 16), (4, 48), (1, 64), (3, 32)])
def test_decode_attention_against_fp64(heads, d, dtype):
    """softmax(scale q K^T) V of one query row over the first `len` cache rows, against fp64 on the storage-rounded inputs:
    err <= attn_ref.FLOOR (1e-5 fp32, 2^-6 bf16: what the one-launch attention is held to).  len in LENS with Lmax = 1024
    and an appended row, plus the cross-attention form (len = Lmax = 11, caches read-only); B in {1, 5}; q | k_new | v_new
    as column blocks of one buffer in half the cases.  Cache rows >= len hold NaN; afterwards row len-1 holds k_new / v_new
    bit for bit and every other row, two guard rows around each cache included, is bit-identical."""
    cases = [(length, LMAX, True) for length in LENS] + [(11, 11, False)]
    worst, n = 0.0, 0
    for B in (1, 5):
        for length, lmax, append in cases:
            packed = n % 2 == 0
            n += 1
            e, bad = _one_decode_call(B, heads, d, length, lmax, append, packed, dtype, "decode")
            print("decode_attn heads %d d %d %s B %d len %4d/%4d %s %s: err %.3e" % (
                heads, d, "bf16" if dtype == BF16 else "fp32", B, length, lmax, "append" if append else "read  ",
                "packed" if packed else "dense ", e))
            assert not bad, (B, length, lmax, append, packed, bad)
            assert e <= attn_ref.FLOOR[dtype], (B, length, lmax, append, packed, e)
            worst = max(worst, e)
    print("worst %.3e (floor %.3e)" % (worst, attn_ref.FLOOR[dtype]))


def test_greedy_next_picks_the_lowest_index_and_builds_the_next_row():
    from focus_amd import ops
    dv = dev()
    g = torch.Generator().manual_seed(5)
    B, V, D = 7, 777, 40
    dic, pe = torch.randn(V, D, generator=g), torch.randn(D, generator=g)
    for dtype in (F32, BF16):
        lg = torch.randn(B, V, generator=g).to(dtype)
        lg[0, 5] = lg[0, 700] = 9.0                      # a tie across two threads' strides: the lower index
        lg[1, 776] = 9.0                                 # the last column
        lg[2, 0] = 9.0
        lg[3, 300] = lg[3, 301] = lg[3, 44] = 9.0
        table = torch.full((B, 3), -1, dtype=torch.long, device=dv)
        x = ops.greedy_next(lg.to(dv), dic.to(dv), pe.to(dv), table[:, 1])
        want = lg.float().argmax(dim=-1)
        assert want[0] == 5 and want[1] == 776 and want[2] == 0 and want[3] == 44
        assert torch.equal(table[:, 1].cpu(), want)
        assert bool((table[:, 0] == -1).all()) and bool((table[:, 2] == -1).all())
        assert x.dtype == dtype and torch.equal(x.cpu(), (dic[want] + pe).to(dtype))


@pytest.mark.parametrize("dtype,tol", [(BF16, 3e-2), (F32, 1e-3)], ids=["bf16", "fp32"])
def test_decoder_steps_match_the_full_pass(oracle, dtype, tol):
    """320 teacher-forced TransformerDecoder.step calls at the width of the BASELINE shape (d_model 192, 4 heads of 48, 11
    slots), stacked, against oracle.transformer_decoder in fp32 on the CPU on the same storage-rounded inputs: the criteria
    of the full pass (test_gpu_steve.py).  320 tokens cross the 64- and 256-key boundaries of the kernel's key loop."""
    from focus_amd.slowfast.models.STEVE.transformer import TransformerDecoder
    d = dev()
    B, T, K, D, H, NB = 3, 320, 11, 192, 4, 2
    torch.manual_seed(3)
    m = TransformerDecoder(NB, T, D, H, dropout=0.0).to(d).eval()
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(B, T, D, generator=g).to(dtype)
    e0 = torch.randn(B, K, D, generator=g).to(dtype)
    p = {"tf." + k: v.detach().float().cpu() for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    yr = oracle.transformer_decoder(p, "tf", x0.float(), e0.float(), H, NB)
    x, e = x0.to(d), e0.to(d)
    with torch.no_grad():
        cache = m.init_cache(e, T)
        assert len(cache) == NB and cache[0][0].shape == (B, T, D) and cache[0][2].shape == (B, K, D)
        rows = [m.step(x[:, t:t + 1], cache, t) for t in range(T)]
    assert rows[0].shape == (B, 1, D) and rows[0].dtype == dtype
    close(torch.cat(rows, dim=1), yr, tol, "stacked decoder steps")
    m.train()
    with pytest.raises(AssertionError, match="evaluation path"):
        m.step(x[:, :1], cache, 0)


# ------------------------------------------------------------------------------------------------
# STEVE.decode
# ------------------------------------------------------------------------------------------------
HEADS, BLOCKS, GEN = 2, 2, 16                            # of the configuration below: (IMG_SIZE / 4)^2 = 16 tokens


def _steve_small(mixed):
    """The configuration of tests/test_gpu_steve.py::_steve_small: what the steve_forward_small fixture was made with."""
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import MODEL_REGISTRY
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "STEVE"
    cfg.NUM_GPUS = 1
    cfg.TRAIN.MIXED_PRECISION = mixed
    s = cfg.SLOTS
    s.NUM_ITERS, s.NUM_SLOTS, s.CNN_HID_SIZE, s.SIZE, s.DIM, s.MLP_HID_SIZE, s.IMG_SIZE, s.VOCAB_SIZE = 2, 3, 16, 16, 32, 32, 16, 32
    s.NUM_PREDICTOR_BLOCKS, s.NUM_PREDICTOR_HEADS = 1, 2
    s.DECODER.DIM, s.DECODER.NUM_BLOCKS, s.DECODER.NUM_HEADS = 32, 2, 2
    return cfg, MODEL_REGISTRY.get("STEVE")(cfg)


def _model(mixed):
    from conftest import load_golden
    _, p = load_golden("steve_forward_small")
    _, m = _steve_small(mixed)
    missing, unexpected = m.load_state_dict(p, strict=False)
    assert not unexpected and all(k.endswith("self_attn_mask") for k in missing), (missing, unexpected)
    return m.to(dev()).eval(), p


def _slots():
    return torch.randn(6, 3, 16, generator=torch.Generator().manual_seed(2))


def _decode_capturing_ids(m, slots, monkeypatch):
    """m.decode(slots) -> (image, the [B, GEN] token ids it turned into one-hot planes)."""
    from focus_amd.slowfast.models.STEVE import steve
    seen = []
    real = steve.F.one_hot
    with monkeypatch.context() as mp:
        mp.setattr(steve.F, "one_hot", lambda t, n: (seen.append(t.detach().cpu().clone()), real(t, n))[1])
        img = m.decode(slots)
    assert len(seen) == 1 and seen[0].shape == (slots.shape[0], GEN) and seen[0].dtype == torch.long
    return img, seen[0]


def test_greedy_decode_fp32_reproduces_the_fp64_tokens(oracle, monkeypatch):
    """fp32 STEVE.decode (the steve_forward_small weights, N(0,1) slots of seed 2) generates exactly the 6 x 16 greedy ids of
    the fp64 incremental reference, and the image of the loop it replaces (FOCUS_STEVE_DECODE_CACHE=0) to 1e-3.
    Exactness is a fair demand: the smallest top-2 logit gap of the fp64 reference over these 96 decisions is 1.234e-2 at
    |logit| <= 3.07 (re-checked below, >= 1e-3 asserted), four orders above an fp32 kernel's logit error."""
    monkeypatch.delenv("FOCUS_STEVE_DECODE_CACHE", raising=False)
    m, p = _model(False)
    assert m.decode_cache
    slots = _slots()
    p64 = {k: v.double() for k, v in p.items()}
    sp = slots.double() @ p64["steve_encoder.slot_proj.weight"].t()
    ids_ref, logits_ref = decode_ref.greedy_tokens(oracle, p64, sp, HEADS, BLOCKS, GEN)
    gap = decode_ref.top2_gap(logits_ref)
    print("fp64 reference: smallest top-2 gap %.3e, max |logit| %.2f" % (gap, float(logits_ref.abs().max())))
    assert gap >= 1e-3
    img, ids = _decode_capturing_ids(m, slots.to(dev()), monkeypatch)
    assert img.shape == (6, 3, 16, 16)
    assert torch.equal(ids, ids_ref), (ids != ids_ref).nonzero()
    monkeypatch.setenv("FOCUS_STEVE_DECODE_CACHE", "0")
    m0, _ = _model(False)
    assert not m0.decode_cache
    img0, ids0 = _decode_capturing_ids(m0, slots.to(dev()), monkeypatch)
    assert torch.equal(ids0, ids_ref)
    close(img, img0, 1e-3, "image: cached loop against the full-prefix loop")


def test_greedy_decode_bf16_stays_within_the_margin_of_the_oracle(oracle, monkeypatch):
    """bf16 ids cannot be compared step by step (one near-tie changes everything after it).  Instead: one causal
    teacher-forced pass of the oracle (fp32, bf16-rounded weight matrices and inputs) over the ids the cached path
    generated gives every step's reference logits, and every generated id must be within m of that step's best logit, no
    position exempt.  m = 4 x the largest |logit difference| between the existing full-prefix bf16 path (dec.tf + head on
    the same ids) and that oracle pass, measured here: 2 for "the chosen and the best token may both be off by the path's
    error" x 2 for the cached path rounding at other points than the full pass.  Figures: trailing comment."""
    from focus_amd import ops
    monkeypatch.delenv("FOCUS_STEVE_DECODE_CACHE", raising=False)
    m, p = _model(True)
    assert m.compute_dtype == BF16 and m.decode_cache
    slots = _slots().to(dev())
    _, ids = _decode_capturing_ids(m, slots, monkeypatch)
    dec = m.steve_decoder
    with torch.no_grad():
        sp = ops.linear(slots.to(BF16), m.steve_encoder.slot_proj.weight)                    # as decode() projects them
        emb = torch.cat([dec.bos.expand(6, -1, -1), dec.dict.dictionary(ids.to(dev()))], dim=1)
        x = dec.pos(emb)[:, :-1].to(BF16)                                                     # the inputs of positions 0 .. 15
        full = ops.linear(dec.tf(x, sp), dec.head.weight).float().cpu()                       # the parent's path on these ids
    pr = {k: (v.bfloat16().float() if v.dim() == 2 and k.endswith(".weight") else v.float()) for k, v in p.items()}
    ref = oracle.transformer_decoder(pr, "steve_decoder.tf", x.float().cpu(), sp.float().cpu(), HEADS, BLOCKS)
    ref = ref @ pr["steve_decoder.head.weight"].t()
    margin = 4.0 * float((full - ref).abs().max())
    chosen = ref.gather(-1, ids.unsqueeze(-1)).squeeze(-1)
    shortfall = float((ref.max(dim=-1).values - chosen).max())
    print("bf16 greedy decode: m = %.3e (4 x %.3e), worst shortfall of a generated id %.3e, ids off the oracle's arg-max "
          "%d / %d" % (margin, margin / 4, shortfall, int((ref.argmax(-1) != ids).sum()), ids.numel()))
    assert margin > 0.0 and shortfall <= margin


def test_decode_takes_the_cached_loop_only_where_it_should(monkeypatch):
    """Knob unset and eval(): 2 x NUM_BLOCKS x gen_len ops.decode_attention calls and no TransformerDecoder.forward.
    FOCUS_STEVE_DECODE_CACHE=0 at construction, or train(): the other way round."""
    from focus_amd import ops
    from focus_amd.slowfast.models.STEVE.transformer import TransformerDecoder
    n = {"attn": 0, "fwd": 0}
    real_attn, real_fwd = ops.decode_attention, TransformerDecoder.forward

    def attn(*a, **k):
        n["attn"] += 1
        return real_attn(*a, **k)

    def fwd(self, *a, **k):
        n["fwd"] += 1
        return real_fwd(self, *a, **k)

    monkeypatch.setattr(ops, "decode_attention", attn)
    monkeypatch.setattr(TransformerDecoder, "forward", fwd)
    slots = _slots()[:2].to(dev())

    def run(m):
        n["attn"] = n["fwd"] = 0
        img = m.decode(slots)
        assert img.shape == (2, 3, 16, 16) and bool(torch.isfinite(img).all())
        return n["attn"], n["fwd"]

    monkeypatch.delenv("FOCUS_STEVE_DECODE_CACHE", raising=False)
    m, _ = _model(False)
    assert run(m) == (2 * BLOCKS * GEN, 0)
    m.train()
    assert run(m) == (0, GEN)
    monkeypatch.setenv("FOCUS_STEVE_DECODE_CACHE", "0")
    m0, _ = _model(False)
    monkeypatch.delenv("FOCUS_STEVE_DECODE_CACHE")       # read once, at construction
    assert run(m0) == (0, GEN)


# Measured on an MI355X (pytest tests/test_gpu_decode_cache.py -m gpu -s):
#
#   test_decode_attention_against_fp64, worst err over the 20 calls of a case   fp32 (floor 1e-5)   bf16 (floor 1.56e-2)
#     heads 2, d 16                                                             2.03e-07            2.85e-03
#     heads 4, d 48                                                             1.95e-07            3.69e-03
#     heads 1, d 64                                                             1.97e-07            3.28e-03
#     heads 3, d 32                                                             1.56e-07            2.60e-03
#   (len = 1 gives 0 in both types: one key, probability 1, the output is the stored value row)
#
#   test_greedy_decode_fp32_reproduces_the_fp64_tokens: smallest top-2 gap of the fp64 reference 1.234e-02, max |logit| 3.07;
#     96 / 96 ids equal, from the cached loop and from the full-prefix loop
#   test_greedy_decode_bf16_stays_within_the_margin_of_the_oracle: m = 7.362e-02 (4 x 1.840e-02, the full-prefix bf16 path
#     against the oracle pass); worst shortfall of a generated id 0.000e+00: all 96 ids are the oracle pass's arg-max
