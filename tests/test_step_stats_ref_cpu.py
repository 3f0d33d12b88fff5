"""No GPU: the twin of csrc/step_stats.hip (tests/step_stats_ref.py) against the pinned mirrors (metrics.topks_correct,
multitask_topks_correct, train.mixup_collapse) and the recorded fixture (tests/golden/metrics.npz); hand-derived cases for
the rules themselves; the mutants of the twin; the two symbols in the header and the library with the refusals they judge
before any launch; and the host side of meters.StepStats on hand-filled CPU tables, two gloo ranks included."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

import mixup_ref
import step_stats_ref as ref
from conftest import GOLDEN, ROOT

VS = (5, 6, 63, 64, 65, 97, 174, 255, 256, 257, 300)
BS = (1, 3, 8)
KS = (1, 5)


def as_torch(rows, bf16):
    t = torch.from_numpy(rows)
    return t.to(torch.bfloat16) if bf16 else t


def counts(preds, labels, ks=KS, bf16=False, mutant=None, **kw):
    acc_i, acc_f = ref.new_acc()
    ref.topk_stats(acc_i, acc_f, preds, labels, ks, bf16=bf16, mutant=mutant, **kw)
    return acc_i[ref.CORRECT:].reshape(3, 4)[:, :len(ks)].tolist()


# ---- twin against the mirrors ------------------------------------------------------------------------------------------------
def test_rows_are_distinct_in_both_dtypes():
    mag = ref.magnitudes()
    assert mag.size == 512 and np.unique(mag).size == 512
    assert np.array_equal(ref.round_bf16(mag), mag)                                  # bf16-exact
    assert np.array_equal(torch.from_numpy(mag).to(torch.bfloat16).float().numpy(), mag)
    rows = ref.tie_free_rows(3, 300, 0)
    assert all(np.unique(r).size == 300 for r in rows)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("V", VS)
def test_twin_matches_topks_correct_on_tie_free_rows(V, bf16):
    from focus_amd.slowfast.utils import metrics
    for B in BS:
        rows = ref.tie_free_rows(B, V, seed=V * 10 + B)
        rows2 = ref.tie_free_rows(B, V, seed=V * 10 + B + 5)
        g = np.random.RandomState(V + B)
        l, l2 = g.randint(0, V, B), g.randint(0, V, B)
        p, p2 = as_torch(rows, bf16), as_torch(rows2, bf16)
        tl, tl2 = torch.from_numpy(l), torch.from_numpy(l2)
        want = [int(x) for x in metrics.topks_correct(p, tl, KS)]
        assert counts((rows,), (l,), bf16=bf16)[0] == want == counts((rows,), (l,), bf16=bf16)[2]
        want2 = [int(x) for x in metrics.topks_correct(p2, tl2, KS)]
        both = [int(x) for x in metrics.multitask_topks_correct((p, p2), (tl, tl2), KS)]
        assert counts((rows, rows2), (l, l2), bf16=bf16) == [want, want2, both]


def test_twin_matches_the_recorded_reference_counts():
    z = np.load(os.path.join(GOLDEN, "metrics.npz"), allow_pickle=False)
    s, l, s2, l2 = z["scores"], z["labels"], z["scores2"], z["labels2"]
    got = counts((s, s2), (l, l2))
    assert got[0] == [int(x) for x in z["topk"]] and got[2] == [int(x) for x in z["multitask"]]
    assert counts((s,), (l,))[0] == [int(x) for x in z["topk"]]


def mixup_cases():
    for V in (6, 64, 65, 97, 174, 257, 300):
        for B in (2, 3, 8):
            for lam in (0.3, 0.8):
                for bf16 in (False, True):
                    yield V, B, lam, bf16


def test_twin_matches_mixup_collapse_where_torch_defines_the_order():
    """Only rows on which torch.topk's order is specified are compared: the label row's top three strictly ordered (a
    mixed pair of two classes) and the collapsed winner's score equal to no other entry.  296 of the 364 rows are kept; the
    others are self-paired rows (the middle row of an odd batch, or equal labels drawn by chance) and bf16 sum collisions."""
    from focus_amd import train
    from focus_amd.slowfast.utils import metrics
    kept = total = 0
    for V, B, lam, bf16 in mixup_cases():
        rows = ref.tie_free_rows(B, V, seed=V + B)
        l = np.random.RandomState(0).randint(0, V, B)
        dense = mixup_ref.target(l, V, lam, 0.1)
        cp, cl = train.mixup_collapse(as_torch(rows, bf16), torch.from_numpy(dense))
        cpf = cp.float().numpy()
        for r in range(B):
            total += 1
            top3 = np.sort(dense[r])[::-1][:3]
            ordered = top3[0] > top3[1] > top3[2]
            winner_alone = (cpf[r] == cpf[r, cl[r]]).sum() == 1
            if not (ordered and winner_alone):
                continue
            kept += 1
            want = [int(x) for x in metrics.topks_correct(cp[r:r + 1], cl[r:r + 1], KS)]
            assert counts((rows[r:r + 1],), (dense[r:r + 1],), bf16=bf16)[0] == want, (V, B, lam, bf16, r)
    assert kept >= 0.75 * total, (kept, total)


# ---- the rules by hand -------------------------------------------------------------------------------------------------------
def ranks(pred, label, bf16=False, mutant=None):
    return ref.row_rank(np.float32(pred), label if np.ndim(label) == 0 else np.float32(label), bf16, mutant)


def test_rules_by_hand():
    nan = float("nan")
    # a tie at the k boundary: the lower index comes first
    assert ranks([1, 2, 2, 0], 2) == 1 and ranks([1, 2, 2, 0], 1) == 0
    assert counts((np.float32([[1, 2, 2, 0]]),), ([2],), ks=(1, 2))[0] == [0, 1]
    assert counts((np.float32([[1, 2, 2, 0]]),), ([1],), ks=(1, 2))[0] == [1, 1]
    assert ranks([0.0, -0.0], 1) == 1                                                # -0 == 0: the index decides
    # NaN is the greatest; two NaNs do not beat each other; +inf is an ordinary value
    assert ranks([nan, 3, 1], 1) == 1 and ranks([nan, 3, 1], 0) == 0 and ranks([nan, nan, 1], 1) == 0
    assert ranks([float("inf"), nan, 1], 0) == 1 and ranks([nan, nan, 1], 2) == 2
    # a label outside the row is never correct; k = V takes every labelled row
    assert ranks([1, 2], 2) == -1 and ranks([1, 2], -1) == -1
    assert counts((ref.tie_free_rows(4, 5, 1),), ([0, 1, 4, 5],), ks=(1, 5))[0][1] == 3
    # single-peak label rows (lam = 1, or a pair of one class): second is the lowest index of the rest
    onehot = mixup_ref.target(np.array([1]), 4, 1.0, 0.1)[0]
    assert ref.greatest(onehot) == 1 and ref.greatest(onehot, skip=1) == 0
    assert ranks([4, -1, 3, 2], onehot) == 0                                         # [0, 3, 3, 2]: the tie goes to index 1
    assert ranks([4, -1, 3, 2], onehot, mutant="keep_second") == 1                   # [4, 3, 3, 2]
    assert ranks([4, -1, 3, 2], onehot, mutant="ties_high") == 2                     # second = 3: [4, 1, 3, 0]
    # the collapsed sum rounds once to bf16: 1 + 2^-8 is half way and goes to the even 1.0, which index 0 then beats
    lab = np.float32([0, 0.2, 0.7, 0.1])
    assert ranks([1.0, 2.0 ** -8, 1.0, -3], lab, bf16=True) == 1
    assert ranks([1.0, 2.0 ** -8, 1.0, -3], lab, bf16=False) == 0
    assert ranks([1.0, 2.0 ** -8, 1.0, -3], lab, bf16=True, mutant="no_round") == 0


def test_scalars_by_hand():
    acc_i, acc_f = ref.new_acc()
    losses = [np.float32(0.1), np.float32(float("inf")), np.float32(float("nan")), np.float32(0.3), np.float32(float("nan"))]
    tot = w = np.float64(0)
    for s, l in enumerate(losses):
        ref.topk_stats(acc_i, acc_f, losses=(l, None, np.float32(2.0)), batch=3 + s)
        tot, w = tot + np.float64(l), w + np.float64(l) * (3 + s)
    assert acc_i[:4].tolist() == [5, 3 + 4 + 5 + 6 + 7, 1, 2] and not acc_i[4:].any()       # inf passes, the first NaN stays
    assert np.isnan(acc_f[0]) and acc_f[1] == 0 and acc_f[2] == 10.0 and acc_f[5] == 2.0 * 25
    a2 = ref.new_acc()
    ref.topk_stats(*a2, losses=(np.float32(0.1),), batch=2)
    ref.topk_stats(*a2, losses=(np.float32(0.7),), batch=5)
    assert a2[1][0] == np.float64(np.float32(0.1)) + np.float64(np.float32(0.7))
    assert a2[1][3] == np.float64(np.float32(0.1)) * 2 + np.float64(np.float32(0.7)) * 5
    ref.topk_stats(*a2, losses=(np.float32(0.7),), batch=0)                                 # B <= 0: nothing
    assert a2[0][:2].tolist() == [2, 7]


def view_tables(NV, C):
    return np.zeros((NV, C), np.float32), np.zeros(NV, np.int64), np.zeros(NV, np.int64)


def test_view_accumulate_by_hand():
    preds = np.float32([[1, 5], [1e8, 2], [-1e8, 7], [3, 3]])
    ids, labels = np.array([2, 3, 2, 0]), np.array([4, 4, 4, 1])
    vp, vl, cc = view_tables(2, 2)
    assert ref.view_accumulate(preds, ids, labels, 2, vp, vl, cc) == 0
    assert vp.tolist() == [[3, 3], [0, 14]] and vl.tolist() == [1, 4] and cc.tolist() == [1, 3]   # (1 + 1e8) - 1e8 = 0 in fp32
    vp2, vl2, cc2 = view_tables(2, 2)
    ref.view_accumulate(preds, ids, labels, 2, vp2, vl2, cc2, mutant="descending")
    assert vp2.tolist() == [[3, 3], [1, 14]]
    # the split of the batches does not matter
    vp3, vl3, cc3 = view_tables(2, 2)
    for s in (slice(0, 1), slice(1, 4)):
        ref.view_accumulate(preds[s], ids[s], labels[s], 2, vp3, vl3, cc3)
    assert np.array_equal(vp3, vp) and np.array_equal(cc3, cc)
    # conflict: only against a non-zero stored label; the label is written either way; out of range: skipped, bit 1
    assert ref.view_accumulate(preds[:1], [0], [2], 2, vp, vl, cc) == 1 and vl[0] == 2
    vz = view_tables(2, 2)
    assert ref.view_accumulate(preds[:2], [0, 1], [0, 3], 2, *vz) == 0 and vz[1][0] == 3
    assert ref.view_accumulate(preds[:2], [4, -1], [3, 3], 2, *vz) == 2 and vz[2].tolist() == [2, 0]
    vm = view_tables(1, 2)
    ref.view_accumulate(np.float32([[-1, 2], [float("nan"), 1], [5, -4]]), [0, 1, 0], [1, 1, 1], 3, *vm, mode="max")
    assert np.isnan(vm[0][0, 0]) and vm[0][0, 1] == 2                               # zeros start the maximum, a NaN stays


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_some_case_tells_every_mutant_apart(mutant):
    differs = False
    lab = np.float32([[0, 0.2, 0.7, 0.1]])
    for preds, labels, bf16 in (((np.float32([[1, 2, 2, 0]]),), ([2],), False),
                                ((np.float32([[1.0, 2.0 ** -8, 1.0, -3]]),), (lab,), True),
                                ((np.float32([[1, 5, -1, 0]]),), (lab,), False),         # [1, 0, 4, 0], or [1, 5, 4, 0]
                                ((np.float32([[1, 2]]), np.float32([[1, 2]])), ([1], [0]), False)):
        differs |= counts(preds, labels, ks=(1,), bf16=bf16) != counts(preds, labels, ks=(1,), bf16=bf16, mutant=mutant)
    preds = np.float32([[1, 5], [1e8, 2], [-1e8, 7]])
    a, b = view_tables(1, 2), view_tables(1, 2)
    ref.view_accumulate(preds, [0, 1, 2], [1, 1, 1], 3, *a)
    ref.view_accumulate(preds, [0, 1, 2], [1, 1, 1], 3, *b, mutant=mutant)
    differs |= not np.array_equal(a[0], b[0])
    assert differs, mutant


# ---- the C ABI, no GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def test_header_declares_and_library_exports(built):
    from focus_amd import _lib
    decl = _lib.parse_header()
    L = ctypes.CDLL(built)
    for n in ("focus_topk_stats", "focus_view_accumulate"):
        assert n in decl and hasattr(L, n), n
    assert len(decl["focus_topk_stats"][1]) == 26 and len(decl["focus_view_accumulate"][1]) == 15
    assert _lib.lib().focus_abi_version() == 2


def test_entry_points_refuse_before_launching(built):
    """Host pointers and no GPU: every refusal below is judged before a launch, and nothing is written."""
    from focus_amd import _lib, ops
    from focus_amd.slowfast.utils import meters
    lib = _lib.lib()
    F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    NULL, SHAPE, DTYPE = -5, -1, -2
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    a += -a % 16
    p = ctypes.c_void_p(a)

    def topk(heads=1, B=4, h0=(p, F32, 10, 10, p, 0), h1=(p, BF16, 12, 16, p, 0), dense=0, ks=(1, 5), losses=(p, None, None),
             acc=(p, p)):
        k4 = list(ks)[:4] + [0] * (4 - len(ks))
        return lib.focus_topk_stats(heads, B, *h0, *h1, dense, len(ks), *k4, *losses, *acc, None)

    assert topk(acc=(None, p)) == NULL and topk(acc=(p, None)) == NULL
    assert topk(heads=0, acc=(None, p)) == NULL
    assert topk(h0=(None, F32, 10, 10, p, 0)) == NULL and topk(h0=(p, F32, 10, 10, None, 0)) == NULL
    assert topk(heads=2, h1=(None, F32, 10, 10, p, 0)) == NULL and topk(heads=2, h1=(p, F32, 10, 10, None, 0)) == NULL
    assert topk(heads=-1) == SHAPE and topk(heads=3) == SHAPE
    assert topk(ks=()) == SHAPE and topk(ks=(1, 2, 3, 4, 5)) == SHAPE
    assert topk(ks=(5, 1)) == SHAPE and topk(ks=(1, 1)) == SHAPE and topk(ks=(0, 1)) == SHAPE
    assert topk(ks=(1, 11)) == SHAPE and topk(heads=2, ks=(1, 11)) == SHAPE           # above V of head 0
    assert topk(heads=2, h0=(p, F32, 20, 20, p, 0), ks=(1, 13)) == SHAPE              # above V of head 1
    assert topk(h0=(p, F32, 0, 10, p, 0), ks=(1,)) == SHAPE
    assert topk(h0=(p, F32, 1, 1, p, 1), ks=(1,), dense=1) == SHAPE                   # dense labels need V >= 2
    assert topk(h0=(p, F32, 10, 9, p, 0)) == SHAPE                                    # a stride below V
    assert topk(h0=(p, F32, 10, 10, p, 9), dense=1) == SHAPE
    assert topk(h0=(p, FP8, 10, 10, p, 0)) == DTYPE and topk(heads=2, h1=(p, 7, 12, 16, p, 0)) == DTYPE
    assert topk(B=0) == 0 and topk(B=-3) == 0 and topk(heads=0, B=0) == 0             # without a launch
    view = lib.focus_view_accumulate
    good = [p, F32, 4, 13, 13, p, p, 6, 7, 0, p, p, p, p, None]
    for i in (0, 5, 6, 10, 11, 12, 13):
        args = list(good)
        args[i] = None
        assert view(*args) == NULL, i
    for i, v in ((7, 0), (3, 0), (4, 12), (9, 2), (9, -1)):                           # num_clips, C, ld < C, the mode
        args = list(good)
        args[i] = v
        assert view(*args) == SHAPE, (i, v)
    assert view(*(good[:1] + [FP8] + good[2:])) == DTYPE
    assert view(*(good[:2] + [0] + good[3:])) == 0 and view(*(good[:2] + [-1] + good[3:])) == 0
    assert bytes(buf) == bytes(1 << 12)
    x = torch.rand(4, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_stats(torch.zeros(16, dtype=torch.int64), torch.zeros(8, dtype=torch.float64), x, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_accumulate(x, torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 2, torch.zeros(2, 10),
                            torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meters.StepStats("cpu").update(x, torch.zeros(4, dtype=torch.int64), torch.zeros(()))


# ---- StepStats on the host -----------------------------------------------------------------------------------------------
def fill(st, steps, samples, correct, loss_sum, loss_weighted, nan=None):
    st.acc_i.zero_()
    st.acc_f.zero_()
    st.acc_i[0], st.acc_i[1] = steps, samples
    if nan is not None:
        st.acc_i[2], st.acc_i[3] = 1, nan
    for h, row in enumerate(correct):
        for j, c in enumerate(row):
            st.acc_i[4 + 4 * h + j] = c
    for i, (s, w) in enumerate(zip(loss_sum, loss_weighted)):
        st.acc_f[i], st.acc_f[3 + i] = s, w


def test_step_stats_windows_and_epoch_on_hand_filled_tables():
    from focus_amd.slowfast.utils import meters
    st = meters.StepStats("cpu")
    fill(st, 2, 16, [[4, 12], [0, 0], [4, 12]], [3.0], [20.0])
    w = st.read()
    assert w == {"top1_err": 75.0, "top5_err": 25.0, "loss": 1.5, "samples": 16, "steps": 2}
    assert not st.acc_i.any() and not st.acc_f.any()                                   # the window was reset
    fill(st, 1, 4, [[4, 4], [0, 0], [4, 4]], [0.5], [2.0])
    assert st.read(reset=False)["top1_err"] == 0.0 and st.acc_i[0] == 1                # a look that keeps the window
    assert st.read() == {"top1_err": 0.0, "top5_err": 0.0, "loss": 0.5, "samples": 4, "steps": 1}
    e = st.epoch_stats()
    assert e == {"top1_err": 60.0, "top5_err": 20.0, "loss": 22.0 / 20, "samples": 20, "steps": 3}
    st.reset_epoch()
    assert st.epoch_stats()["samples"] == 0


def test_step_stats_ek_keys_and_slot_losses():
    from focus_amd.slowfast.utils import meters
    st = meters.StepStats("cpu", multitask=True)
    fill(st, 4, 32, [[16, 24], [8, 16], [4, 12]], [8.0, 4.0, 2.0], [64.0, 32.0, 16.0])
    w = st.read()
    assert set(w) == {"verb_top1_acc", "verb_top5_acc", "noun_top1_acc", "noun_top5_acc", "action_top1_acc", "action_top5_acc",
                      "verb_loss", "noun_loss", "loss", "samples", "steps"}
    assert (w["verb_top1_acc"], w["noun_top5_acc"], w["action_top1_acc"], w["action_top5_acc"]) == (50.0, 50.0, 12.5, 37.5)
    assert (w["loss"], w["verb_loss"], w["noun_loss"]) == (2.0, 1.0, 0.5)
    assert st.epoch_stats()["verb_loss"] == 1.0 and st.epoch_stats()["action_top5_acc"] == 37.5
    sl = meters.StepStats("cpu", ks=(), aux_names=("mse", "cross_entropy"))
    fill(sl, 2, 6, [], [3.0, 1.0, 2.0], [9.0, 3.0, 6.0])
    assert sl.read() == {"loss": 1.5, "mse": 0.5, "cross_entropy": 1.0, "samples": 6, "steps": 2}


def test_step_stats_raises_the_reference_error_on_a_latched_nan():
    from focus_amd.slowfast.utils import meters
    st = meters.StepStats("cpu")
    fill(st, 3, 12, [[1, 2], [0, 0], [1, 2]], [1.0], [4.0])
    st.read()
    fill(st, 5, 20, [[1, 2], [0, 0], [1, 2]], [float("nan")], [float("nan")], nan=2)
    with pytest.raises(RuntimeError, match=r"ERROR: Got NaN losses \(step 5\)"):       # 3 steps read before + step 2 of the window
        st.read()
    assert not st.acc_i.any()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from focus_amd.slowfast.utils import meters
    st = meters.StepStats("cpu")
    fill(st, 2, 8 + 8 * rank, [[2 + rank, 6], [0, 0], [2 + rank, 6]], [1.0 + rank], [8.0 + 16 * rank])
    w = st.read()
    ok = w == {"top1_err": 100.0 * (24 - 5) / 24, "top5_err": 50.0, "loss": 3.0 / 4, "samples": 24, "steps": 2}
    alone = meters.StepStats("cpu")
    fill(alone, 2, 8, [[2, 6], [0, 0], [2, 6]], [1.0], [8.0])
    ok &= alone.read(reduce=False)["samples"] == 8
    fill(st, 3, 12, [[1, 2], [0, 0], [1, 2]], [1.0], [4.0], nan=1 if rank == 1 else None)
    try:
        st.read()
        ok = False
    except RuntimeError as e:                                       # a NaN on rank 1 is seen by both
        ok &= str(e) == ("ERROR: Got NaN losses (step 3)" if rank == 1 else "ERROR: Got NaN losses (on another rank)")
    with open(out + str(rank), "w") as f:
        f.write("%d" % ok)
    dist.barrier()
    dist.destroy_process_group()


def test_step_stats_two_ranks_gloo(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "res")
    mp.spawn(_gloo_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert open(out + "0").read() == "1" and open(out + "1").read() == "1"
