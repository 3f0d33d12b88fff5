"""STEVE.decode (greedy autoregressive generation, steve.py:359-381) with the key/value cache on and off, in one process.

The BASELINE decoder (IMG_SIZE 128 -> 1024 tokens, d_model 192, 4 heads of 48, 8 blocks, 11 slots, vocabulary 4096, bf16):
the cached loop (TransformerDecoder.step + ops.decode_attention + ops.greedy_next) and the full-prefix loop it replaces
(FOCUS_STEVE_DECODE_CACHE=0) alternate on the same model and the same slots at --seqs sequences, then the cached loop runs
alone at --big-seqs (8 clips x 24 frames, what reconstruct_autoregressive hands it).  Each measurement is one decode()
between two device events followed by a synchronise.  Both loops are warmed up first on a model of the same width at
IMG_SIZE 32 (64 tokens), which loads every kernel either loop launches; the same small model counts the library's launches
per token.  The full-prefix loop at 1024 tokens is the long leg: it runs --full-reps times (default once).

usage: python tools/decode_bench.py [--seqs 24] [--big-seqs 192] [--img-size 128] [--full-reps 1]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SLOTS, WIDTH, HEADS, BLOCKS, VOCAB = 11, 192, 4, 8, 4096


def build(img_size, dev):
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import MODEL_REGISTRY
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "STEVE"
    cfg.NUM_GPUS = 1
    cfg.TRAIN.MIXED_PRECISION = True
    sl = cfg.SLOTS
    sl.NUM_ITERS, sl.NUM_SLOTS, sl.CNN_HID_SIZE, sl.SIZE, sl.DIM, sl.MLP_HID_SIZE, sl.IMG_SIZE, sl.VOCAB_SIZE = (
        3, SLOTS, 64, WIDTH, WIDTH, 768, img_size, VOCAB)
    sl.NUM_PREDICTOR_BLOCKS, sl.NUM_PREDICTOR_HEADS, sl.PREDICTOR_DROPOUT = 1, 4, 0.0
    sl.DECODER.DIM, sl.DECODER.NUM_BLOCKS, sl.DECODER.NUM_HEADS, sl.DECODER.DROPOUT = WIDTH, BLOCKS, HEADS, 0.1
    torch.manual_seed(0)
    return MODEL_REGISTRY.get("STEVE")(cfg).to(dev).eval()


def timed_decode(m, slots, cache):
    """One decode() between two device events -> (milliseconds, image)."""
    m.decode_cache = cache
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    with torch.no_grad():
        img = m.decode(slots)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), img


def library_calls(m, slots, cache):
    """Entry points of libfocus_amd.so called by one decode() (each enqueues one kernel; a split-K GEMM two)."""
    from focus_amd import _lib
    L = _lib.lib()
    names = [n for n in _lib.parse_header() if n not in ("focus_strerror", "focus_abi_version", "focus_gemm_last_kernel")
             and not n.endswith("_ok") and not n.endswith("_bytes")]
    n = [0]
    real = {k: getattr(L, k) for k in names}

    def counted(f):
        def g(*a):
            n[0] += 1
            return f(*a)
        return g

    for k, f in real.items():
        setattr(L, k, counted(f))
    try:
        timed_decode(m, slots, cache)
    finally:
        for k, f in real.items():
            setattr(L, k, f)
    return n[0]


def kv_bytes(seqs, tokens):
    """Bytes of cached keys and values the cached loop's attention reads over a whole decode (bf16)."""
    per_row = 2 * WIDTH * 2                              # K and V rows
    return BLOCKS * seqs * per_row * (tokens * (tokens + 1) // 2 + tokens * SLOTS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=24)
    ap.add_argument("--big-seqs", type=int, default=192)
    ap.add_argument("--img-size", type=int, default=128)
    ap.add_argument("--full-reps", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    slots_of = lambda n: torch.randn(n, SLOTS, WIDTH, generator=g).to(dev)

    small = build(32, dev)
    ws = slots_of(a.seqs)
    for cache in (True, False, True, False):             # warm-up of both loops
        timed_decode(small, ws, cache)
    wt = (32 // 4) ** 2
    calls = {c: library_calls(small, ws, c) for c in (True, False)}
    print("library launches per token (counted over %d tokens): cached %.1f, full-prefix %.1f (+ ATen: argmax, embedding, "
          "2 cat, position add, cast)" % (wt, calls[True] / wt, calls[False] / wt))

    m = build(a.img_size, dev)
    tokens = (a.img_size // 4) ** 2
    slots = slots_of(a.seqs)
    res = {"cached_ms": [], "full_ms": []}
    img_c = img_f = None
    for _ in range(a.full_reps):
        ms, img_c = timed_decode(m, slots, True)
        res["cached_ms"].append(ms)
        ms, img_f = timed_decode(m, slots, False)
        res["full_ms"].append(ms)
    ms, img_c = timed_decode(m, slots, True)
    res["cached_ms"].append(ms)
    best_c, best_f = min(res["cached_ms"]), min(res["full_ms"])
    same = float((img_c == img_f).float().mean())
    print("%d sequences x %d tokens, bf16: cached %s ms, full-prefix %s ms (alternated; best %.1f vs %.1f: x%.1f)" % (
        a.seqs, tokens, ["%.1f" % x for x in res["cached_ms"]], ["%.1f" % x for x in res["full_ms"]], best_c, best_f,
        best_f / best_c))
    print("  cached: %.3f ms per token, K/V read %.2f GB over the decode = %.1f GB/s" % (
        best_c / tokens, kv_bytes(a.seqs, tokens) / 1e9, kv_bytes(a.seqs, tokens) / 1e6 / best_c))
    print("  fraction of identical output pixels, cached vs full-prefix (bf16 near-ties may fork a sequence): %.4f" % same)
    out = {"workload": "STEVE.decode greedy generation, bf16", "tokens": tokens, "seqs": a.seqs, "cached_ms": round(best_c, 2),
           "full_prefix_ms": round(best_f, 2), "speedup": round(best_f / best_c, 2),
           "launches_per_token_cached": round(calls[True] / wt, 1), "launches_per_token_full": round(calls[False] / wt, 1)}
    if a.big_seqs > 0:
        big = slots_of(a.big_seqs)
        t = [timed_decode(m, big, True)[0] for _ in range(2)]
        gb = kv_bytes(a.big_seqs, tokens) / 1e9
        print("%d sequences x %d tokens, bf16: cached %s ms (%.3f ms per token), K/V read %.2f GB = %.1f GB/s" % (
            a.big_seqs, tokens, ["%.1f" % x for x in t], min(t) / tokens, gb, gb * 1e3 / min(t)))
        out.update({"big_seqs": a.big_seqs, "big_cached_ms": round(min(t), 2), "big_kv_gbps": round(gb * 1e3 / min(t), 1)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
