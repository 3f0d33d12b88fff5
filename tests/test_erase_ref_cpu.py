"""CPU-side checks of the random-erasing path: the mirror RandomErasing class and the twin planner of tests/erase_ref.py against
the reference's recorded draws and outputs (tests/golden/random_erasing.npz), the statistics of the twin's normal values, the
fp32 restatement of the kernel's formula against the bound erase_ref derives (and three mutants against both), and the
argument checks of ops.random_erase_ and focus_random_erase that need no device (no launch happens)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import erase_ref

NULL, SHAPE, DTYPE, ALIGN = -5, -1, -2, -3


@pytest.fixture(scope="module")
def z():
    return erase_ref.fixture()


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def case_input(z, tag):
    what = erase_ref.CASES[tag][1]
    if what == "image":
        return torch.from_numpy(z["image"].copy())
    clip = torch.from_numpy(z["clip"].copy())
    return clip.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3) if what == "view" else clip


def case_frames(tag):
    return None if erase_ref.CASES[tag][1] == "image" else erase_ref.T


def rows_of(items):
    return np.array([[it[k] for k in ("t0", "t1", "top", "left", "h", "w")] for it in items], dtype=np.int64).reshape(-1, 6)


def test_fixture_reaches_every_case(z):
    rects = {t: z[t + ".rects"] for t in erase_ref.CASES}
    assert rects["gate_closed"].shape == (0, 6) and np.array_equal(z["gate_closed.out"], z["clip"])
    for t in ("one_const", "one_rand", "one_pixel", "image"):
        assert rects[t].shape == (1, 6) and z[t + ".attempts"].tolist() == [1] and rects[t][0, 3] % 2 == 1
    assert {erase_ref.CASES[t][0]["mode"] for t in erase_ref.CASES} == {"const", "rand", "pixel"}
    assert z["retry.attempts"][0] > 1
    assert rects["count2_clean"].shape == (2, 6) and (rects["count2_clean"][:, 0] == erase_ref.T // 2).all()
    assert np.array_equal(z["count2_clean.out"][:erase_ref.T // 2], z["clip"][:erase_ref.T // 2])
    assert rects["count3_overlap"].shape == (3, 6) and erase_ref.overlaps(rects["count3_overlap"].tolist())
    assert (rects["count3_overlap"][:, 0] == erase_ref.T // 3).all()
    pf = rects["per_frame"]
    assert (pf[:, 1] - pf[:, 0] == 1).all() and len(set(pf[:, 0].tolist())) >= 2 and len(set(pf[:, 0].tolist())) < erase_ref.T
    assert z["image.out"].shape == (erase_ref.C, erase_ref.H, erase_ref.W)
    assert (z["one_const.out"][:, :, 1:10, 1:6] == 0).all()


@pytest.mark.parametrize("tag", list(erase_ref.CASES))
def test_mirror_on_cpu_equals_the_reference_bit_for_bit(z, tag):
    from focus_amd.slowfast.datasets.random_erasing import RandomErasing
    x = case_input(z, tag)
    seed = int(z[tag + ".seed"])
    random.seed(seed)
    torch.manual_seed(seed)
    got = RandomErasing(device="cpu", **erase_ref.CASES[tag][0])(x)
    assert got is x and x.dtype == torch.float32
    assert np.array_equal(x.contiguous().numpy(), z[tag + ".out"])
    assert random.random() == float(z[tag + ".next_random"])


@pytest.mark.parametrize("tag", list(erase_ref.CASES))
def test_plan_draws_the_references_rectangles_and_leaves_its_state(z, tag):
    from focus_amd.slowfast.datasets.random_erasing import RandomErasing
    kw = erase_ref.CASES[tag][0]
    seed = int(z[tag + ".seed"])
    random.seed(seed)
    items = RandomErasing(device="cpu", **kw).plan(case_frames(tag), erase_ref.H, erase_ref.W)
    assert random.random() == float(z[tag + ".next_random"])
    assert np.array_equal(rows_of(items), z[tag + ".rects"])
    random.seed(seed)                                                      # the twin, which shares no code with the class
    rows, attempts = erase_ref.plan(kw, case_frames(tag), erase_ref.H, erase_ref.W, True)
    assert random.random() == float(z[tag + ".next_random"])
    assert np.array_equal(rows, z[tag + ".rects"]) and attempts == z[tag + ".attempts"].tolist()


def test_plan_and_twin_agree_on_seeds_the_fixture_does_not_hold():
    from focus_amd.slowfast.datasets.random_erasing import RandomErasing
    kws = [dict(probability=0.25, mode="pixel", max_count=1, num_splits=1), dict(probability=0.9, max_count=3, num_splits=3),
           dict(probability=0.7, max_count=2, cube=False), dict(probability=1.0, min_count=2, max_count=2, min_area=0.2, max_area=0.9)]
    for kw in kws:
        for n, h, w in [(8, 224, 224), (4, 10, 14), (None, 7, 5), (3, 2, 2)]:
            for seed in range(40):
                random.seed(seed)
                a = rows_of(RandomErasing(**kw).plan(n, h, w))
                sa = random.random()
                random.seed(seed)
                b = erase_ref.plan(kw, n, h, w)
                assert np.array_equal(a, b) and random.random() == sa


def test_constructor_keeps_the_references_defaults():
    from focus_amd.slowfast.datasets.random_erasing import RandomErasing
    import math
    e = RandomErasing()
    assert (e.probability, e.min_area, e.max_area, e.min_count, e.max_count, e.num_splits, e.device, e.cube) == (
        0.5, 0.02, 1 / 3, 1, 1, 0, "cuda", True)
    assert e.log_aspect_ratio == (math.log(0.3), math.log(1 / 0.3)) and e.mode == "const"
    assert RandomErasing(mode="RAND").mode == "rand" and RandomErasing(mode="Pixel").per_pixel
    with pytest.raises(AssertionError):
        RandomErasing(mode="noise")
    import focus_amd.slowfast as sf
    import sys
    sf.install_as_slowfast()
    assert sys.modules["slowfast.datasets.random_erasing"].RandomErasing is RandomErasing


# ---- the generator -------------------------------------------------------------------------------------------------
S0, S1 = 0x1234abcd, -0x0badf00d           # the second word negative: the seed tensor is int32
GRID = (2, 4, 4, 128, 256)                 # item ordinal, frame, channel, y, x: 2^20 draws


@pytest.fixture(scope="module")
def draws():
    o, t, c, y, x = np.meshgrid(*[np.arange(n) for n in GRID], indexing="ij")
    ha, hb = erase_ref.hashes(S0, S1, o, 1, t, c, erase_ref.position(y, x))
    return ha, hb, (x & 1) == 1, erase_ref.normals(ha, hb, (x & 1) == 1)


def statistics(v):
    """[(name, |statistic - expectation| / its standard error)] of a GRID-shaped array of would-be N(0,1) values."""
    n = v.size
    out = [("mean", abs(v.mean()) * np.sqrt(n)), ("variance", abs(v.var() - 1.0) / np.sqrt(2.0 / n))]
    p = 0.6826894921370859
    out.append(("P(|z|<1)", abs((np.abs(v) < 1).mean() - p) / np.sqrt(p * (1 - p) / n)))
    for axis, name in enumerate(("item", "frame", "channel", "y", "x")):
        a, b = np.moveaxis(v, axis, 0)[:-1].ravel(), np.moveaxis(v, axis, 0)[1:].ravel()
        out.append(("lag-1 " + name, abs(np.corrcoef(a, b)[0, 1]) * np.sqrt(a.size)))
    return out


def test_twin_normals_pass_the_statistics(draws):
    _ha, _hb, _odd, v = draws
    assert v.size == 2 ** 20 and np.isfinite(v).all() and np.abs(v).max() <= erase_ref.R_MAX
    for name, ratio in statistics(v):
        print("%-14s %.2f standard errors" % (name, ratio))
        assert ratio < 5.0, name
    flat = erase_ref.normals(*erase_ref.hashes(S0, S1, 0, np.arange(64)[:, None, None], np.arange(64)[None, :, None],
                                               np.arange(256)[None, None, :], erase_ref.FLAT))
    assert abs(flat.mean()) * np.sqrt(flat.size) < 5.0 and abs(flat.var() - 1.0) / np.sqrt(2.0 / flat.size) < 5.0


def test_generator_depends_on_every_coordinate_and_seed_word():
    assert int(erase_ref.position(5, 6)) == int(erase_ref.position(5, 7)) == (5 << 16) | 3      # a column pair shares a word
    a, b = erase_ref.normals(*erase_ref.hashes(S0, S1, 0, 0, 0, 0, erase_ref.position(5, 6)), odd=np.array([False, True]))
    assert a != b and abs(np.hypot(a, b) ** 2 / -2.0 - np.log((float(erase_ref.hashes(S0, S1, 0, 0, 0, 0, (5 << 16) | 3)[0] >> np.uint64(9)) + 0.5) / 2 ** 23)) < 1e-12
    base = dict(s0=S0, s1=S1, ord_=1, clip=2, t=3, c=1, p=int(erase_ref.position(5, 6)))
    ref = erase_ref.hashes(**base)
    for k in base:
        other = erase_ref.hashes(**dict(base, **{k: base[k] + 1}))
        assert int(other[0]) != int(ref[0]) or int(other[1]) != int(ref[1]), k
    assert int(erase_ref.position(32767, 32767)) != erase_ref.FLAT


def test_fp32_formula_stays_inside_the_derived_bound_and_the_mutants_do_not(draws):
    ha, hb, odd, v = draws
    assert abs(erase_ref.BOUND - 4.81e-6) < 1e-8
    err = np.abs(erase_ref.normals_f32(ha, hb, odd).astype(np.float64) - v).max()
    print("fp32 restatement: max |dz| = %.3g = %.3f of the bound %.3g" % (err, err / erase_ref.BOUND, erase_ref.BOUND))
    assert err <= erase_ref.BOUND
    mutants = {"sine for cosine": erase_ref.normals_f32(ha, hb, odd, sine=True),
               "dropped half in the uniform": erase_ref.normals_f32(ha, hb, odd, drop_half=True),
               "second seed word ignored": erase_ref.normals_f32(ha, erase_ref.mix32(ha), odd)}
    for name, m in mutants.items():
        m = m.astype(np.float64)
        finite = np.isfinite(m)
        worst = np.abs(m - v)[finite].max() / erase_ref.BOUND
        stats = max(r for _n, r in statistics(np.where(finite, m, 0.0)))
        print("%-28s max |dz| = %.3g bounds, worst statistic %.2f standard errors, %d non-finite" % (
            name, worst, stats, (~finite).sum()))
        assert worst > 1.0 or stats >= 5.0 or not finite.all(), name


def test_bf16_half_ulp():
    v = np.array([1.0, 1.9999, 2.0, -3.5, 0.0, 5.7])
    assert erase_ref.bf16_half_ulp(v).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -6]
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0), dtype=torch.float32)
    err = (x.to(torch.bfloat16).double() - x.double()).abs().numpy()
    assert (err <= erase_ref.bf16_half_ulp(x.double().numpy())).all()


def test_expected_lets_the_last_item_of_a_clip_win():
    rows = erase_ref.table([(1, 0, 2, 0, 0, 3, 3), (0, 0, 1, 1, 1, 2, 2), (1, 1, 2, 1, 1, 3, 3)])
    assert rows[:, 0].tolist() == [0, 1, 1] and rows[:, 7].tolist() == [0, 0, 1]
    written, vals, owner = erase_ref.expected((2, 2, 2, 5, 5), rows, "pixel", S0, S1)
    assert owner[1, 0, 1, 1, 1] == 2 and owner[1, 0, 0, 1, 1] == 1 and owner[1, 1, 1, 0, 0] == 1 and owner[0, 0, 1, 1, 1] == -1
    assert written.sum() == 2 * (9 + 9 + 5) + 2 * 4 and (vals[~written] == 0).all()
    a = erase_ref.normals(*erase_ref.hashes(S0, S1, 1, 1, 1, 0, erase_ref.position(2, 2)))
    b = erase_ref.normals(*erase_ref.hashes(S0, S1, 1, 1, 1, 0, erase_ref.position(2, 3)), odd=True)
    assert vals[1, 0, 1, 2, 2] == a and vals[1, 0, 1, 2, 3] == b and a != b


# ---- refusals that need no device ------------------------------------------------------------------------------------
def item(**kw):
    return dict(dict(clip=0, t0=0, t1=2, top=1, left=1, h=2, w=3), **kw)


def test_ops_validates_every_item_on_the_host():
    from focus_amd import ops
    x = torch.zeros(2, 3, 4, 6, 8)                                        # a CPU tensor: nothing below reaches the device
    bad = [item(clip=2), item(clip=-1), item(t0=-1), item(t0=2, t1=2), item(t1=5), item(h=0), item(w=0), item(top=-1),
           item(top=5), item(left=6), item(left=-2), item(h=2.0), item(w=True), dict(clip=0), (0, 0, 2, 1, 1, 2, 3)]
    for it in bad:
        with pytest.raises(ValueError):
            ops.random_erase_(x, [item(), it], "pixel", "BCTHW")
    with pytest.raises(ValueError, match="frames"):
        ops.random_erase_(x, [item(t1=4)], "const", "BTCHW")             # T is 3 in that layout
    with pytest.raises(ValueError, match="layout"):
        ops.random_erase_(x, [item()], "const", "BHWC")
    with pytest.raises(ValueError, match="mode"):
        ops.random_erase_(x, [item()], "noise", "BCTHW")
    with pytest.raises(ValueError, match="5-d"):
        ops.random_erase_(x[0], [item()], "const", "BCTHW")
    with pytest.raises(ValueError, match="at most %d" % ops.ERASE_MAX_PER_CLIP):
        ops.random_erase_(x, [item()] * (ops.ERASE_MAX_PER_CLIP + 1), "const", "BCTHW")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.random_erase_(x, [item()], "const", "BCTHW")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.random_erase_(x, [], "const", "BCTHW")


def test_erase_table_orders_the_items_of_a_clip():
    from focus_amd import ops
    items = [item(clip=1, left=0), item(clip=0, left=1), item(clip=1, left=2), item(clip=1, left=3)]
    rec, most = ops.erase_table(items, 2, 4, 6, 8)
    assert rec.dtype == np.int32 and rec.shape == (4, 8) and most == 3
    assert rec[:, 0].tolist() == [0, 1, 1, 1] and rec[:, 4].tolist() == [1, 0, 2, 3] and rec[:, 7].tolist() == [0, 0, 1, 2]
    assert np.array_equal(rec, erase_ref.table([tuple(it[k] for k in ops.ERASE_ITEM_FIELDS) for it in items]))
    rec, most = ops.erase_table([], 2, 4, 6, 8)
    assert rec.shape == (0, 8) and most == 0


def test_erase_clips_returns_its_input_when_the_config_erases_nothing():
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.datasets import device_sampling
    cfg = get_cfg()
    x = torch.zeros(2, 3, 2, 4, 4)
    assert device_sampling.erase_clips(cfg, x) is x                       # AUG.ENABLE is off (or AUG is absent)
    cfg.merge_from_list(["AUG.ENABLE", "True", "AUG.RE_PROB", "0.0"])
    assert device_sampling.erase_clips(cfg, x) is x
    cfg.merge_from_list(["AUG.ENABLE", "False", "AUG.RE_PROB", "1.0"])
    assert device_sampling.erase_clips(cfg, x) is x


def test_entry_point_validates_before_launching(built):
    from focus_amd import _lib
    lib = _lib.lib()
    F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr, odd2, odd1 = ctypes.c_void_p(a), ctypes.c_void_p(a + 2), ctypes.c_void_p(a + 1)

    def call(x=ptr, dtype=F32, B=2, T=4, C=3, H=16, W=16, sb=3072, sc=1024, st=256, items=ptr, n=1, per=1, mode=2, seed=ptr):
        return lib.focus_random_erase(x, dtype, B, T, C, H, W, sb, sc, st, items, n, per, mode, seed, None)
    assert call(x=None) == NULL and call(items=None) == NULL
    assert call(seed=None, mode=2) == NULL and call(seed=None, mode=1) == NULL
    assert call(x=None, n=0) == NULL                                      # NULL is judged first
    assert call(n=0) == 0 and call(n=-3, H=0, dtype=FP8) == 0             # nothing to do: nothing else is judged
    assert call(mode=3) == SHAPE and call(mode=-1) == SHAPE and call(mode=3, seed=None) == SHAPE
    for kw in (dict(B=0), dict(T=0), dict(C=0), dict(H=0), dict(W=0), dict(H=32769), dict(W=32769), dict(T=65536),
               dict(C=65536), dict(n=65536), dict(per=0), dict(per=65), dict(sb=0), dict(sc=255), dict(st=255)):
        assert call(**kw) == SHAPE, kw
    assert call(dtype=FP8) == DTYPE and call(dtype=7) == DTYPE
    assert call(dtype=FP8, H=0) == SHAPE and call(dtype=FP8, x=odd1) == DTYPE     # the order: SHAPE, DTYPE, ALIGN
    assert call(x=odd2) == ALIGN and call(x=odd1, dtype=BF16) == ALIGN
    assert bytes(buf) == bytes(1 << 12)


def test_library_exports_the_symbol_and_the_header_names_the_modes(built):
    from focus_amd import _lib, ops
    decl = _lib.parse_header()
    L = ctypes.CDLL(built)
    assert "focus_random_erase" in decl and hasattr(L, "focus_random_erase")
    assert decl["focus_random_erase"][1] == [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_int64] * 3 + [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    src = open(_lib.HEADER).read()
    assert "FOCUS_ERASE_CONST = 0, FOCUS_ERASE_RAND = 1, FOCUS_ERASE_PIXEL = 2" in src
    assert "#define FOCUS_ERASE_MAX_PER_CLIP %d" % ops.ERASE_MAX_PER_CLIP in src
    assert ops.ERASE_MODES == ("const", "rand", "pixel")
    assert _lib.lib().focus_abi_version() == 2
