"""TRAIN.FP8_ACTIVATIONS measured in one process: (1) per HR GEMM shape (tests/test_gpu_fp8.py HR_SHAPES) the bf16 ws
kernel, the fp8-weight instance (BFP8) and the MX GEMM, interleaved rounds after warm-up, with the fc1 GELU (+ saved
pre-activation) and fc2 residual epilogues where the model uses them, plus the MX quantiser on that shape's input;
(2) the HR training step (bench.py's bench_hr loop: make_cfg(hr=True) + train_step) at batch 4 and 16 with FP8_WEIGHTS
alone (A) against FP8_WEIGHTS + FP8_ACTIVATIONS (B), alternated A/B/A/B, every round reported.

    python tools/fp8_act_bench.py [--out profiles/r04_fp8_act_bench]            # both parts; <out>.json
    python tools/fp8_act_bench.py --step-only --keyed --batch 4 --rounds 1      # one keyed step loop (for rocprofv3)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from focus_amd import ops  # noqa: E402

HR_SHAPES = [(14116, 768, 768), (14116, 2304, 768), (14116, 3072, 768), (14116, 768, 3072), (3529, 768, 768)]
EPI = {(14116, 3072, 768): "gelu+aux (fc1)", (14116, 768, 3072): "residual (fc2)"}


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us


def gemm_table(rounds, reps):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for (M, N, K) in HR_SHAPES:
        a = torch.randn(M, K, device=dev, generator=g).bfloat16()
        w = torch.randn(N, K, device=dev, generator=g) * K ** -0.5
        bias = torch.randn(N, device=dev, generator=g)
        epi = EPI.get((M, N, K), "bias")
        aux = torch.empty(M, N, device=dev, dtype=torch.bfloat16) if epi.startswith("gelu") else None
        res = torch.randn(M, N, device=dev, generator=g).bfloat16() if epi.startswith("residual") else None
        act = ops.EPI_GELU if aux is not None else ops.EPI_NONE
        wb = w.bfloat16()
        wq, sc = ops.shadow_fp8(w)
        xq, xs = ops.mx_quantize(a)
        variants = {
            "bf16_ws": lambda: ops.mm_nt(a, wb, bias=bias, residual=res, aux=aux, epilogue=act),
            "fp8w_ws8": lambda: ops.mm_nt(a, wq, bias=bias, residual=res, aux=aux, epilogue=act, b_scale=sc),
            "mx": lambda: ops.mm_nt_mx(xq, xs, wq, sc, bias=bias, residual=res, aux=aux, epilogue=act),
            "quant": lambda: ops.mx_quantize(a),
        }
        for fn in variants.values():                  # warm-up (and the one-time LDS attribute of each instance)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(rounds):                       # variants alternate inside every round
            for k, fn in variants.items():
                t[k].append(_time(fn, reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        fl = 2.0 * M * N * K
        qbytes = M * K * 2 + M * K + M * K // 32
        row = {"shape": [M, N, K], "epilogue": epi,
               "us": {k: round(v, 2) for k, v in med.items()},
               "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()},
               "tflops": {k: round(fl / (med[k] * 1e-6) / 1e12, 1) for k in ("bf16_ws", "fp8w_ws8", "mx")},
               "mx_over_fp8w": round(med["fp8w_ws8"] / med["mx"], 3),
               "mx_plus_quant_over_fp8w": round(med["fp8w_ws8"] / (med["mx"] + med["quant"]), 3),
               "quant_tb_per_s": round(qbytes / (med["quant"] * 1e-6) / 1e12, 2)}
        rows.append(row)
        print("%-20s %-15s bf16 %7.1f us  fp8w %7.1f us  mx %7.1f us (%.1f TF/s, x%.2f vs fp8w)  quant %6.1f us %.2f TB/s" % (
            "x".join(map(str, (M, N, K))), epi, med["bf16_ws"], med["fp8w_ws8"], med["mx"], row["tflops"]["mx"],
            row["mx_over_fp8w"], med["quant"], row["quant_tb_per_s"]), flush=True)
        del a, w, wb, xq, xs, aux, res
        ops.drop_caches()
    return rows


def _model(batch, keyed, dev):
    import bench
    from focus_amd.slowfast.models import build_model
    from focus_amd.slowfast.models.losses import get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    from focus_amd.train import synthetic_batch
    cfg = bench.make_cfg(1, batch, hr=True)
    cfg.merge_from_list(["TRAIN.FP8_WEIGHTS", True, "TRAIN.FP8_ACTIVATIONS", bool(keyed)])
    torch.manual_seed(0)
    model = build_model(cfg, gpu_id=dev.index)
    model.train()
    opt = construct_optimizer(model, cfg)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    inputs, labels, meta = synthetic_batch(cfg, batch, dev, seed=77)
    return model, opt, loss_fun, inputs, labels, meta, cfg


def _steps(st, n):
    from focus_amd.train import train_step
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        _, loss = train_step(*st)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n, float(loss.detach())


def step_ab(batch, rounds, steps, keyed_only=False):
    dev = torch.device("cuda:0")
    arms = ("keyed",) if keyed_only else ("fp8w", "keyed")
    st = {arm: _model(batch, arm == "keyed", dev) for arm in arms}
    for arm in arms:                                  # warm-up
        _steps(st[arm], 2)
    ms = {arm: [] for arm in arms}
    loss = {}
    for _ in range(rounds):
        for arm in arms:                              # A/B/A/B
            t, loss[arm] = _steps(st[arm], steps)
            ms[arm].append(round(t, 3))
    rec = {"batch": batch, "steps_per_round": steps, "ms_per_step_rounds": ms,
           "final_loss": {k: round(v, 4) for k, v in loss.items()}}
    for arm in arms:
        v = ms[arm]
        rec[arm] = {"median_ms": round(statistics.median(v), 3), "min_ms": min(v), "max_ms": max(v),
                    "clips_per_s_median": round(batch / (statistics.median(v) * 1e-3), 2)}
    if not keyed_only:
        a, b = rec["fp8w"], rec["keyed"]
        spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
        rec["keyed_speedup_median"] = round(a["median_ms"] / b["median_ms"], 4)
        rec["difference_ms"] = round(a["median_ms"] - b["median_ms"], 3)
        rec["within_spread"] = abs(rec["difference_ms"]) <= spread
        print("HR step batch %d: fp8w %s ms, fp8w+fp8act %s ms (rounds); median x%.3f%s" % (
            batch, ms["fp8w"], ms["keyed"], rec["keyed_speedup_median"],
            " (inside the spread)" if rec["within_spread"] else ""), flush=True)
    else:
        print("HR step batch %d keyed: %s ms" % (batch, ms["keyed"]), flush=True)
    del st
    ops.drop_caches()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the record to <out>.json")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--gemm-only", action="store_true")
    ap.add_argument("--keyed", action="store_true", help="step part: the keyed model only")
    ap.add_argument("--batch", type=int, default=None)
    a = ap.parse_args()
    from focus_amd.build import source_hash
    rec = {"tool": "tools/fp8_act_bench.py", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    print("source %s on %s" % (rec["source_hash"], rec["device"]), flush=True)
    if not a.step_only:
        rec["gemm"] = gemm_table(a.rounds, a.reps)
    if not a.gemm_only:
        batches = [a.batch] if a.batch else [int(b) for b in a.batches.split(",")]
        rec["hr_step"] = []
        for b in batches:
            try:
                rec["hr_step"].append(step_ab(b, a.rounds, a.steps, keyed_only=a.keyed))
            except torch.cuda.OutOfMemoryError as e:
                rec["hr_step"].append({"batch": b, "failed": repr(e)[:200]})
                ops.drop_caches()
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
