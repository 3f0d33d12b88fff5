"""Pre-LN transformer encoder (slot predictor) and decoder (autoregressive token decoder) of STEVE (mirror of
slowfast/models/STEVE/transformer.py:4-193).  Attention runs as strided batched GEMMs + a row softmax through the C
ABI (ops.small_attention: plain, causal, or cross-attention over the slots); Linear / LayerNorm / FFN are the fused HIP
ops of the hot path.  TransformerDecoder.init_cache / step generate one token at a time against cached keys and values
(ops.decode_attention, csrc/decode_attn.hip): the evaluation path of STEVE.decode."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from focus_amd import ops

from .utils import linear


class MultiHeadAttention(nn.Module):
    """transformer.py:4-50.  attn_mask: None or the decoder's upper-triangular bool mask (applied as `causal`).
    Dropout (attention probabilities and output) is drawn with ATen in training mode."""

    def __init__(self, d_model, num_heads, dropout=0.0, gain=1.0):
        super().__init__()
        assert d_model % num_heads == 0, "d_model must be divisible by num_heads"
        self.d_model = d_model
        self.num_heads = num_heads
        self.attn_dropout = nn.Dropout(dropout)
        self.output_dropout = nn.Dropout(dropout)
        self.proj_q = linear(d_model, d_model, bias=False)
        self.proj_k = linear(d_model, d_model, bias=False)
        self.proj_v = linear(d_model, d_model, bias=False)
        self.proj_o = linear(d_model, d_model, bias=False, gain=gain)

    def forward(self, q, k, v, attn_mask=None, residual=None):
        B, T, _ = q.shape
        S = k.shape[1]
        causal = attn_mask is not None
        if causal:
            assert attn_mask.shape == (T, S) and T == S, "only the decoder's causal mask is supported"
        d = self.d_model // self.num_heads
        p = self.attn_dropout.p if self.training else 0.0
        bf16 = q.dtype == torch.bfloat16
        if q is k and k is v and bf16 and ((not causal and T <= 16 and self.d_model % 64 == 0) or d in (32, 48, 64)):
            # self-attention: the three projections are the column blocks of one product, which ops.small_attention's
            # one-launch kernels (the predictor over the slots) and ops.flash_attention (the decoder over the image tokens)
            # read in place
            Q, Kt, V = ops.linear_qkv(q, self.proj_q.weight, self.proj_k.weight, self.proj_v.weight)
        else:
            Q = ops.linear(q, self.proj_q.weight)
            Kt = ops.linear(k, self.proj_k.weight)
            V = ops.linear(v, self.proj_v.weight)
        if (causal or T > 16) and ops.flash_ok(Q, Kt, V, self.num_heads, causal):
            # the decoder (causal over 1024 tokens; cross-attention from them to the slots): no [T, S] probabilities and no
            # dropout mask in memory, the mask is a function of a seed drawn from torch's generator (csrc/flash_attn.hip)
            a = ops.flash_attention(Q, Kt, V, self.num_heads, d ** -0.5, causal=causal, p=p)
        else:
            drop = None
            if p > 0.0:
                drop = F.dropout(torch.ones(B, self.num_heads, T, S, device=q.device, dtype=q.dtype), p, True)
            a = ops.small_attention(Q, Kt, V, self.num_heads, d ** -0.5, causal=causal, drop=drop)
        if self.training and self.output_dropout.p > 0.0:
            return ops.dropout_add(ops.linear(a, self.proj_o.weight), residual, self.output_dropout.p, True)
        return ops.linear(a, self.proj_o.weight, residual=residual)


def _norm(ln, x):
    return ops.layer_norm(x, ln.weight, ln.bias, ln.eps)


def _make_ffn(d_model, gain, dropout):
    """The feed-forward member of both block kinds: indices 0 / 2 hold the Linear layers, 3 the dropout."""
    return nn.Sequential(linear(d_model, 4 * d_model, weight_init="kaiming"), nn.ReLU(),
                         linear(4 * d_model, d_model, gain=gain), nn.Dropout(dropout))


def _ffn(seq, x, residual, training):
    """Linear -> ReLU -> Linear -> Dropout (+ residual): one fused op, the residual in the second GEMM's epilogue."""
    up, down, drop = seq[0], seq[2], seq[3]
    if training and drop.p > 0.0:
        y = ops.mlp(x, up.weight, up.bias, down.weight, down.bias, act=ops.EPI_RELU)
        return ops.dropout_add(y, residual, drop.p, True)          # mask from a seed, rebuilt by the backward (gumbel.hip)
    return ops.mlp(x, up.weight, up.bias, down.weight, down.bias, residual=residual, act=ops.EPI_RELU)


class _BlockStack(nn.Module):
    """`blocks` (the first one flagged is_first) followed by a closing LayerNorm: the shape both transformers share.
    `branches` is the number of residual branches per block; the output projections are scaled by
    (branches * num_blocks) ** -0.5 (transformer.py:101, :175)."""

    def __init__(self, num_blocks, d_model, branches, make_block):
        super().__init__()
        gain = (branches * num_blocks) ** (-0.5) if num_blocks > 0 else 1.0
        self.blocks = nn.ModuleList([make_block(gain, i == 0) for i in range(num_blocks)])
        self.layer_norm = nn.LayerNorm(d_model)

    def forward(self, input, *context):
        for block in self.blocks:
            input = block(input, *context)
        return _norm(self.layer_norm, input)


class TransformerEncoderBlock(nn.Module):
    def __init__(self, d_model, num_heads, dropout=0.0, gain=1.0, is_first=False):
        super().__init__()
        self.is_first = is_first
        self.attn_layer_norm = nn.LayerNorm(d_model)
        self.attn = MultiHeadAttention(d_model, num_heads, dropout, gain)
        self.ffn_layer_norm = nn.LayerNorm(d_model)
        self.ffn = _make_ffn(d_model, gain, dropout)

    def forward(self, input):
        ln = self.attn_layer_norm
        if self.is_first:       # the residual stream itself is normalised (:75-78)
            input = _norm(ln, input)
            input = self.attn(input, input, input, residual=input)
        else:
            input, x = ops.layer_norm_fork(input, ln.weight, ln.bias, ln.eps)
            input = self.attn(x, x, x, residual=input)
        fl = self.ffn_layer_norm
        input, x = ops.layer_norm_fork(input, fl.weight, fl.bias, fl.eps)   # (residual-path gradient added in the LN backward)
        return _ffn(self.ffn, x, input, self.training)


class TransformerEncoder(_BlockStack):
    """transformer.py:96-114 (two residual branches per block)."""

    def __init__(self, num_blocks, d_model, num_heads, dropout=0.0):
        super().__init__(num_blocks, d_model, 2,
                         lambda gain, first: TransformerEncoderBlock(d_model, num_heads, dropout, gain, is_first=first))


class TransformerDecoderBlock(nn.Module):
    """transformer.py:117-166: causal self-attention, cross-attention over the slots, FFN; pre-LN (the first block
    normalises the residual stream itself)."""

    def __init__(self, max_len, d_model, num_heads, dropout=0.0, gain=1.0, is_first=False):
        super().__init__()
        self.is_first = is_first
        self.self_attn_layer_norm = nn.LayerNorm(d_model)
        self.self_attn = MultiHeadAttention(d_model, num_heads, dropout, gain)
        mask = torch.triu(torch.ones((max_len, max_len), dtype=torch.bool), diagonal=1)
        self.self_attn_mask = nn.Parameter(mask, requires_grad=False)
        self.encoder_decoder_attn_layer_norm = nn.LayerNorm(d_model)
        self.encoder_decoder_attn = MultiHeadAttention(d_model, num_heads, dropout, gain)
        self.ffn_layer_norm = nn.LayerNorm(d_model)
        self.ffn = _make_ffn(d_model, gain, dropout)

    def forward(self, input, encoder_output):
        T = input.shape[1]
        ln = self.self_attn_layer_norm
        mask = self.self_attn_mask[:T, :T]
        if self.is_first:
            input = _norm(ln, input)
            input = self.self_attn(input, input, input, mask, residual=input)
        else:
            x = _norm(ln, input)
            input = self.self_attn(x, x, x, mask, residual=input)
        x = _norm(self.encoder_decoder_attn_layer_norm, input)
        input = self.encoder_decoder_attn(x, encoder_output, encoder_output, residual=input)
        return _ffn(self.ffn, _norm(self.ffn_layer_norm, input), input, self.training)


class TransformerDecoder(_BlockStack):
    """transformer.py:169-193 (three residual branches per block); forward(input, encoder_output)."""

    def __init__(self, num_blocks, max_len, d_model, num_heads, dropout=0.0):
        super().__init__(num_blocks, d_model, 3, lambda gain, first: TransformerDecoderBlock(
            max_len, d_model, num_heads, dropout, gain, is_first=first))

    # ---- generation: one token per call against cached keys and values (STEVE.decode) ----
    def init_cache(self, encoder_output, max_len):
        """The state of `step` for encoder_output [B, S, D] and up to max_len generated positions: a list with one
        (self_k, self_v, cross_k, cross_v) per block -- the zero-initialised self-attention caches [B, max_len, D] that
        `step` fills row by row, and the keys / values of the slots, projected once -- which also carries the step's
        buffers and its launches with fixed arguments (ops.Prepared), built here once."""
        B, _, D = encoder_output.shape
        dt, dev = encoder_output.dtype, encoder_output.device
        own = encoder_output.new_zeros(len(self.blocks), 2, B, max_len, D)
        cache = _DecoderCache()
        new = lambda n: torch.empty(B, n, device=dev, dtype=dt)
        cache.res = (new(D), new(D))                     # the residual stream, written alternately (no in-place product)
        y, qkv, q2, cache.att = new(D), new(3 * D), new(D), new(D)
        cache.q, cache.k_new, cache.v_new, cache.q2 = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], q2
        cache.stats = torch.empty(2, B, device=dev, dtype=torch.float32)
        cache.stream = torch.cuda.current_stream().cuda_stream      # the prepared launches are bound to it
        cur = 0                                          # which of cache.res holds the residual stream
        for i, block in enumerate(self.blocks):
            sa, ca, ffn = block.self_attn, block.encoder_decoder_attn, block.ffn
            ck, cv = ops.linear_kv(encoder_output, ca.proj_k.weight, ca.proj_v.weight)
            cache.append((own[i, 0], own[i, 1], ck, cv))
            w = lambda p: ops.shadow(p, dt)
            hid = new(ffn[0].weight.shape[0])
            pre, mid, post = ops.Prepared(), ops.Prepared(), ops.Prepared()
            ln = block.self_attn_layer_norm
            if i == 0:       # is_first: step() normalises its input into res[0], which is residual stream and branch input
                assert block.is_first
                pre.linear(cache.res[0], ops.stacked_weights((sa.proj_q.weight, sa.proj_k.weight, sa.proj_v.weight), dt), qkv)
            else:
                assert not block.is_first
                pre.layer_norm(cache.res[cur], ln.weight, ln.bias, ln.eps, y)
                pre.linear(y, ops.stacked_weights((sa.proj_q.weight, sa.proj_k.weight, sa.proj_v.weight), dt), qkv)
            mid.linear(cache.att, w(sa.proj_o.weight), cache.res[cur ^ 1], residual=cache.res[cur])
            cur ^= 1
            ln = block.encoder_decoder_attn_layer_norm
            mid.layer_norm(cache.res[cur], ln.weight, ln.bias, ln.eps, y)
            mid.linear(y, w(ca.proj_q.weight), q2)
            post.linear(cache.att, w(ca.proj_o.weight), cache.res[cur ^ 1], residual=cache.res[cur])
            cur ^= 1
            ln = block.ffn_layer_norm
            post.layer_norm(cache.res[cur], ln.weight, ln.bias, ln.eps, y)
            post.linear(y, w(ffn[0].weight), hid, bias=ffn[0].bias, epilogue=ops.EPI_RELU)
            post.linear(hid, w(ffn[2].weight), cache.res[cur ^ 1], bias=ffn[2].bias, residual=cache.res[cur])
            cur ^= 1
            cache.launches.append((pre, mid, post))
        cache.last = cur
        return cache

    def step(self, x_t, cache, t):
        """x_t [B, 1, D]: the position-embedded input at index t -> the row forward() produces at index t, [B, 1, D].
        Row t of every block's self-attention cache is written; calls must come in the order t = 0, 1, 2, ...
        Per block: LN -> q | k | v in one product -> ops.decode_attention with append -> proj_o + residual -> LN -> proj_q
        -> ops.decode_attention over the slots' cache -> proj_o + residual -> LN -> FFN + residual."""
        assert not self.training, "TransformerDecoder.step is the evaluation path (the dropouts draw nothing here)"
        assert not torch.is_grad_enabled() or not x_t.requires_grad, "TransformerDecoder.step is inference only"
        B, D = cache.res[0].shape
        assert x_t.shape == (B, 1, D) and x_t.dtype == cache.res[0].dtype
        assert torch.cuda.current_stream().cuda_stream == cache.stream, "step() on another stream than init_cache()"
        x2 = x_t.detach().reshape(B, D)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        first = self.blocks[0].self_attn_layer_norm if len(self.blocks) else None
        if first is not None:        # block 0 normalises the residual stream itself, as in forward()
            ops.layer_norm_into(x2, first.weight, first.bias, first.eps, cache.res[0], cache.stats)
        for block, (sk, sv, ck, cv), (pre, mid, post) in zip(self.blocks, cache, cache.launches):
            heads = block.self_attn.num_heads
            scale = (D // heads) ** -0.5
            pre.run()
            ops.decode_attention(cache.q, cache.k_new, cache.v_new, sk, sv, t + 1, heads, scale, out=cache.att)
            mid.run()
            ops.decode_attention(cache.q2, None, None, ck, cv, ck.shape[1], heads, scale, out=cache.att)
            post.run()
        src = cache.res[cache.last] if first is not None else x2
        out = torch.empty(B, 1, D, device=src.device, dtype=src.dtype)
        ops.layer_norm_into(src, self.layer_norm.weight, self.layer_norm.bias, self.layer_norm.eps, out.view(B, D), cache.stats)
        return out


class _DecoderCache(list):
    """What TransformerDecoder.init_cache returns: the per-block (self_k, self_v, cross_k, cross_v), plus the buffers and
    prepared launches of a step."""

    def __init__(self):
        super().__init__()
        self.launches = []
