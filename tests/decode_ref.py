"""Plain references for greedy generation with cached keys and values (csrc/decode_attn.hip, TransformerDecoder.step,
STEVE.decode).  The checker of tests/test_gpu_decode_cache.py, itself checked without a GPU by
tests/test_decode_ref_cpu.py; the product never imports this, and this imports neither a GPU nor focus_amd.

  decode_attention     one call of focus_decode_attn in fp64: softmax over the first `length` rows of explicit caches
  IncrementalDecoder   oracle.transformer_decoder one position at a time, from the oracle's own pieces
  greedy_tokens        STEVE.decode's token loop over it (arg-max, dictionary row, position row)
"""
import torch


def decode_attention(q, k_cache, v_cache, length, heads, scale):
    """q [B, C], caches [B, Lmax, C] -> softmax(scale q K^T) V per head over rows 0 .. length-1, fp64 [B, C].  Rows
    >= length are not looked at."""
    B, C = q.shape
    d = C // heads
    qh = q.double().view(B, heads, 1, d)
    kh = k_cache[:, :length].double().view(B, length, heads, d).transpose(1, 2)
    vh = v_cache[:, :length].double().view(B, length, heads, d).transpose(1, 2)
    p = torch.softmax(scale * (qh @ kh.transpose(-1, -2)), dim=-1)
    return (p @ vh).reshape(B, C)


class IncrementalDecoder:
    """oracle.transformer_decoder(p, name, x, enc, heads, num_blocks) row by row: step(x_t, t) returns row t of its
    output, given that steps 0 .. t-1 were fed rows 0 .. t-1 of x.  The self-attention keys and values of every block are
    kept in explicit [B, max_len, D] caches, the slots' keys and values are projected once."""

    def __init__(self, oracle, p, name, enc, heads, num_blocks, max_len, eps=1e-5):
        self.o, self.p, self.name, self.heads, self.nb, self.eps = oracle, p, name, heads, num_blocks, eps
        B, _, D = enc.shape
        self.scale = (D // heads) ** -0.5
        self.k = [enc.new_zeros(B, max_len, D) for _ in range(num_blocks)]
        self.v = [enc.new_zeros(B, max_len, D) for _ in range(num_blocks)]
        w = lambda j, which: p["%s.blocks.%d.encoder_decoder_attn.proj_%s.weight" % (name, j, which)]
        self.ck = [enc @ w(j, "k").t() for j in range(num_blocks)]
        self.cv = [enc @ w(j, "v").t() for j in range(num_blocks)]

    def _attend(self, q, k, v, length):
        return decode_attention(q, k, v, length, self.heads, self.scale).to(q.dtype)

    def step(self, x, t):
        """x [B, D] -> [B, D]."""
        o, p = self.o, self.p
        for j in range(self.nb):
            bn = "%s.blocks.%d" % (self.name, j)
            y = o.layer_norm(p, bn + ".self_attn_layer_norm", x, self.eps)
            if j == 0:
                x = y
            self.k[j][:, t] = y @ p[bn + ".self_attn.proj_k.weight"].t()
            self.v[j][:, t] = y @ p[bn + ".self_attn.proj_v.weight"].t()
            a = self._attend(y @ p[bn + ".self_attn.proj_q.weight"].t(), self.k[j], self.v[j], t + 1)
            x = x + a @ p[bn + ".self_attn.proj_o.weight"].t()
            y = o.layer_norm(p, bn + ".encoder_decoder_attn_layer_norm", x, self.eps)
            a = self._attend(y @ p[bn + ".encoder_decoder_attn.proj_q.weight"].t(), self.ck[j], self.cv[j],
                             self.ck[j].shape[1])
            x = x + a @ p[bn + ".encoder_decoder_attn.proj_o.weight"].t()
            y = o.layer_norm(p, bn + ".ffn_layer_norm", x, self.eps)
            x = x + o.linear(p, bn + ".ffn.2", torch.relu(o.linear(p, bn + ".ffn.0", y)))
        return o.layer_norm(p, self.name + ".layer_norm", x, self.eps)


def greedy_tokens(oracle, p, slots, heads, num_blocks, gen_len):
    """STEVE.decode's token loop (steve.py:359-381) on projected slots [B, K, D] with the parameters p of a STEVE model
    (keys steve_decoder.*), in the dtype of p and slots.  -> (ids [B, gen_len] int64, logits [B, gen_len, V])."""
    B = slots.shape[0]
    dec = IncrementalDecoder(oracle, p, "steve_decoder.tf", slots, heads, num_blocks, gen_len)
    pe = p["steve_decoder.pos.pe"][0]
    x = (p["steve_decoder.bos"][0] + pe[:1]).expand(B, -1)
    ids, logits = [], []
    for t in range(gen_len):
        lg = dec.step(x, t) @ p["steve_decoder.head.weight"].t()
        tok = lg.argmax(dim=-1)
        ids.append(tok)
        logits.append(lg)
        x = p["steve_decoder.dict.dictionary.weight"][tok] + pe[t + 1]
    return torch.stack(ids, dim=1), torch.stack(logits, dim=1)


def top2_gap(logits):
    """Smallest difference between the largest and the second largest logit over all rows."""
    top = logits.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())
