"""The AVA evaluation without a GPU: the twin of csrc/ava_eval.hip (tests/ava_eval_ref.py), the host arithmetic of
slowfast/utils/ava_eval_helper.py and meters.AVAMeter against what the reference's own evaluator returned
(tests/golden/ava_eval.npz, written by tests/make_ava_eval_golden.py); the mutants; the tie rule; the readers; the refusals;
all_gather_unaligned and a two-rank AVAMeter over gloo."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import ava_eval_cases as cases
import ava_eval_ref as twin
from conftest import ROOT

from focus_amd.slowfast.utils import ava_eval_helper as helper
from focus_amd.slowfast.utils import meters

TAGS = ("edge", "random")


@pytest.fixture(scope="module")
def golden():
    return cases.load()


@pytest.fixture(scope="module")
def read(golden, tmp_path_factory):
    """Per case: the fixture's arrays and what our readers make of the stored annotation strings."""
    out = {}
    for tag in TAGS:
        c = cases.case(golden, tag)
        root = cases.write_annotations(c, tmp_path_factory.mktemp("ava_" + tag))
        categories, whitelist = helper.read_labelmap(os.path.join(root, "labelmap.pbtxt"))
        excluded = helper.read_exclusions(os.path.join(root, "excl.csv"))
        groundtruth = helper.read_csv(os.path.join(root, "gt.csv"), whitelist)
        out[tag] = dict(c=c, root=root, categories=categories, whitelist=whitelist, excluded=excluded, groundtruth=groundtruth)
    return out


@pytest.fixture(scope="module")
def twin_runs(read):
    """The twin's evaluation of every case, computed once and left unchanged."""
    out = {}
    for tag in TAGS:
        r, c = read[tag], read[tag]["c"]
        out[tag] = twin.evaluate(c["preds"], c["boxes"], c["metadata"], c["names"].tolist(), r["groundtruth"], r["excluded"],
                                 r["whitelist"], max(r["whitelist"]))
    return out


# ---- the readers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_readers_on_the_stored_strings(read, tag):
    r, c = read[tag], read[tag]["c"]
    assert [x["id"] for x in r["categories"]] == c["label_ids"].tolist()
    assert [x["name"] for x in r["categories"]] == c["label_names"].tolist()
    assert r["whitelist"] == set(c["label_ids"].tolist())
    assert sorted(r["excluded"]) == c["excluded"].tolist()
    boxes, labels, scores = r["groundtruth"]
    want = cases.unflatten(c, "gt", False)
    assert list(boxes.keys()) == list(want[0].keys())
    for k in boxes:
        assert boxes[k] == want[0][k] and labels[k] == want[1][k] and scores[k] == want[2][k]       # float64, exact
    assert list(meters.get_ava_mini_groundtruth(r["groundtruth"])[0].keys()) == c["mini_keys"].tolist()
    assert all(int(k.split(",")[1]) % 4 == 0 for k in c["mini_keys"].tolist())
    assert helper.make_image_key("vid", 7) == "vid,0007" and helper.make_image_key("vid", "0904") == "vid,0904"


def test_reader_details(tmp_path):
    p = tmp_path / "d.csv"
    p.write_text("a,0001,0.1,0.2,0.3,0.4,5,0.75\na,0001,0.1,0.2,0.3,0.4,6,0.25\n")
    boxes, labels, scores = helper.read_csv(str(p), {5}, load_score=True)
    assert dict(boxes) == {"a,0001": [[0.2, 0.1, 0.4, 0.3]]} and dict(labels) == {"a,0001": [5]} and dict(scores) == {"a,0001": [0.75]}
    assert helper.read_csv(str(p), None)[1]["a,0001"] == [5, 6] and helper.read_csv(str(p))[2]["a,0001"] == [1.0, 1.0]
    assert helper.read_exclusions(None) == set() and helper.read_exclusions("") == set()
    bad = tmp_path / "bad.csv"
    bad.write_text("a,1,2\n")
    with pytest.raises(AssertionError):
        helper.read_csv(str(bad))
    with pytest.raises(AssertionError):
        helper.read_exclusions(str(bad))


@pytest.mark.parametrize("tag", TAGS)
def test_get_ava_eval_data_and_write_results(read, tag, tmp_path):
    r, c = read[tag], read[tag]["c"]
    got = helper.get_ava_eval_data(c["preds"], c["boxes"], c["metadata"].tolist(), r["whitelist"], video_idx_to_name=c["names"].tolist())
    want = cases.unflatten(c, "det", True)
    assert list(got[0].keys()) == list(want[0].keys())
    for k in want[0]:
        assert got[0][k] == want[0][k] and got[1][k] == want[1][k] and got[2][k] == want[2][k]
    out = tmp_path / "det.csv"
    helper.write_results(got, str(out))
    lines = out.read_text().splitlines()
    assert len(lines) == c["det.labels"].size
    k0 = next(iter(got[0]))
    b, l, s = got[0][k0][0], got[1][k0][0], got[2][k0][0]
    assert lines[0] == "%s,%.03f,%.03f,%.03f,%.03f,%d,%.04f" % (k0, b[1], b[0], b[3], b[2], l, s)
    again = helper.read_csv(str(out), None, load_score=True)
    assert again[1][k0] == got[1][k0]


# ---- the twin and the host arithmetic against the reference ------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_twin_against_the_reference(read, twin_runs, tag):
    c = read[tag]["c"]
    by, counts, n_gt, ap, summary, _ = twin_runs[tag]
    num = c["n_gt"].size
    cases.check_bytes(c, by, "twin " + tag)
    assert np.array_equal(n_gt[:num], c["n_gt"]) and not n_gt[num:].any()
    assert np.array_equal(counts[0], (by != 0).sum(0)) and np.array_equal(counts[1], (by == 2).sum(0))
    cases.check_ap(c, ap, float(summary[0]), "twin " + tag)
    assert summary[1] == (c["n_gt"] > 0).sum()


def test_edge_case_holds_the_situations_it_names(read, twin_runs):
    """The hand-made situations are in the fixture as recorded from the reference, not only in the maker's comments."""
    c = read["edge"]["c"]
    by = twin_runs["edge"][0]
    cases.check_bytes(c, by, "edge")
    keys = cases.row_keys(c)
    a = [r for r, k in enumerate(keys) if k == "vidA,0904"]
    assert len(a) == 4
    assert by[a[0], 0] == 2                                     # the IoU of exactly 0.5 is a true positive
    assert by[a[1], 1] == 2 and by[a[2], 1] == 1 and c["preds"][a[2], 1] > c["preds"][a[1], 1]      # later, higher score: FP
    assert by[a[1], 2] == 2 and by[a[2], 2] == 1               # two equal rows: the first maximum is taken already
    assert not by[a[3]].any()                                   # the invalid box
    assert not by[:, 5].any() and not by[:, 7].any()            # classes outside the whitelist
    assert c["n_gt"][6] == 0 and np.isnan(c["ap"][6])           # whitelisted, no ground truth
    assert not by[[r for r, k in enumerate(keys) if k == "vidB,0012"]].any()                         # excluded
    b = [r for r, k in enumerate(keys) if k == "vidB,0010"]
    assert np.all(by[b][:, [0, 1, 2, 3, 4, 6]] == 1)            # no ground truth: false positives that count
    v = [r for r, k in enumerate(keys) if k == "vidC,0008"]
    assert len(v) == 2 and v[1] - v[0] > 5                      # one key in two batches
    assert c["n_gt"][0] == 2 and c["n_gt"][4] == 5              # vidA,0905 counts although nothing was detected there
    t = [r for r, k in enumerate(keys) if k == "vidA,0906"]
    assert by[t[0], 3] == 2 and by[t[1], 3] == 1               # a tie at 0.5 between two rows: the first one, so the next is late
    tp5 = [int(by[r, 4] == 2) for r, k in enumerate(keys) if k.startswith("vidC")]
    assert sorted(tp5) == [0, 0, 0, 1, 1]                       # threshold pairs: two at or above 0.5 in float64, two below


def test_dict_level_case(golden):
    c = cases.case(golden, "dicts")
    categories = [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}, {"id": 3, "name": "c"}]
    m = helper.run_evaluation(categories, cases.unflatten(c, "gt", True), cases.unflatten(c, "det", True), set(), verbose=False)
    assert m[helper.AP_KEY + "b"] == 0.0 == c["ap"][1]          # ground truth, no detection entry
    assert np.isnan(m[helper.AP_KEY + "c"]) and np.isnan(c["ap"][2])
    assert m[helper.AP_KEY + "a"] == c["ap"][0] and abs(m[helper.MAP_KEY] - c["map"]) <= 2 * cases.U
    assert list(m) == [helper.MAP_KEY] + [helper.AP_KEY + n for n in "abc"]


@pytest.mark.parametrize("tag", TAGS)
def test_host_run_evaluation_and_arrays(read, tag):
    r, c = read[tag], read[tag]["c"]
    num = c["n_gt"].size
    det = cases.unflatten(c, "det", True)
    m = helper.run_evaluation(r["categories"], r["groundtruth"], det, r["excluded"], verbose=False)
    ap = np.full(num, np.nan)
    for cat in r["categories"]:
        ap[cat["id"] - 1] = m[helper.AP_KEY + cat["name"]]
    cases.check_ap(c, ap, m[helper.MAP_KEY], "run_evaluation " + tag)
    res = helper.evaluate_arrays(c["preds"], c["boxes"], c["metadata"], r["excluded"], r["whitelist"], r["categories"],
                                 r["groundtruth"], c["names"].tolist())
    by = np.zeros(c["preds"].shape, dtype=np.uint8)
    v = res["valid"]
    by[res["rows"][v], res["classes"][v] - 1] = 1 + res["tp"][v]
    cases.check_bytes(c, by, "evaluate_arrays " + tag)
    assert np.array_equal(res["n_gt"], c["n_gt"])
    cases.check_ap(c, res["ap"], res["map"], "evaluate_arrays " + tag)


@pytest.mark.parametrize("tag", TAGS)
def test_ava_meter(read, tag, tmp_path, monkeypatch):
    r, c = read[tag], read[tag]["c"]
    cfg = cases.make_cfg(r["root"])
    meter = meters.AVAMeter(len(c["splits"]), cfg, "test")
    assert meter.video_idx_to_name == c["names"].tolist() and meter.class_whitelist == r["whitelist"]
    o = 0
    for n in c["splits"].tolist():
        meter.update_stats(torch.from_numpy(c["preds"][o:o + n]), torch.from_numpy(c["boxes"][o:o + n]),
                           torch.from_numpy(c["metadata"][o:o + n]), loss=0.5, lr=0.1)
        o += n
    monkeypatch.chdir(tmp_path)
    got = meter.finalize_metrics(log=False)
    assert got == meter.full_map and os.listdir(str(tmp_path)) == []           # no CSV files unless asked
    bound = cases.check_ap(c, c["ap"], got, "AVAMeter " + tag)[1]
    assert abs(got - float(c["map"])) <= bound
    stats = meter.log_epoch_stats(3)
    assert stats["map"] == got and stats["cur_epoch"] == "4" and stats["_type"] == "test_epoch"
    meter.finalize_metrics(log=False, write_csv=True)
    assert sorted(os.listdir(str(tmp_path))) == ["detections_latest.csv", "groundtruth_latest.csv"]
    meter.reset()
    assert meter.all_preds == [] and len(meter.loss) == 0
    with pytest.raises(RuntimeError):
        meter.finalize_metrics()


def test_ava_meter_modes(read):
    r, c = read["edge"], read["edge"]["c"]
    rows = (torch.from_numpy(c["preds"]), torch.from_numpy(c["boxes"]), torch.from_numpy(c["metadata"]))
    val = meters.AVAMeter(1, cases.make_cfg(r["root"]), "val")
    val.update_stats(*rows)
    mini = helper.evaluate_ava(*rows, r["excluded"], r["whitelist"], r["categories"],
                               groundtruth=meters.get_ava_mini_groundtruth(r["groundtruth"]), video_idx_to_name=c["names"].tolist())
    assert val.finalize_metrics(log=False) == mini != float(c["map"])
    full = meters.AVAMeter(1, cases.make_cfg(r["root"], full_on_val=True), "val")
    full.update_stats(*rows)
    assert abs(full.finalize_metrics(log=False) - float(c["map"])) <= 16 * cases.U
    train = meters.AVAMeter(1, cases.make_cfg(r["root"]), "train")
    train.update_stats(*rows, loss=1.0, lr=0.01)
    assert train.all_preds == [] and train.lr == 0.01 and train.log_epoch_stats(0) is None
    with pytest.raises(NotImplementedError):
        meters.AVAMeter(1, cases.make_cfg(r["root"]), "other")


# ---- the mutants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", twin.MUTANTS)
def test_mutant_leaves_the_recorded_output(read, mutant):
    """Each mistake moves a per-class AP, or the ground-truth counts, of at least one case further from the reference's
    record than the bound allows."""
    worst = 0.0
    for tag in TAGS:
        r, c = read[tag], read[tag]["c"]
        _, _, n_gt, ap, _, _ = twin.evaluate(c["preds"], c["boxes"], c["metadata"], c["names"].tolist(), r["groundtruth"],
                                             r["excluded"], r["whitelist"], max(r["whitelist"]), mutant=mutant)
        num = c["n_gt"].size
        if not np.array_equal(n_gt[:num], c["n_gt"]) or not np.array_equal(np.isnan(ap[:num]), np.isnan(c["ap"])):
            worst = np.inf
            continue
        off = c["cls.offsets"]
        m = np.array([int(c["cls.tp"][off[k]:off[k + 1]].sum()) for k in range(num)])
        kept = ~np.isnan(c["ap"])
        excess = np.abs(ap[:num][kept] - c["ap"][kept]) - np.maximum(m[kept] - 1, 0) * cases.U
        worst = max(worst, float(excess.max()))
    print(mutant, "leaves the record by", worst)
    assert worst > 1e-6


# ---- the tie rule ------------------------------------------------------------------------------------------------------------
def test_tie_rule_by_hand():
    """Four judged rows of one class with one score: the order is row 3, 2, 1, 0.  Rows 0 and 2 are true positives, n = 2:
    ranks pos = 1 (row 2) and 3 (row 0); p = 1/2, 2/4; envelope 1/2, 1/2; AP = 1/2 * 1/2 + 1/2 * 1/2 = 0.5.  Ascending row
    order would give pos = 0 and 2: p = 1, 2/3, AP = 5/6."""
    scores = np.full((4, 1), 0.25, dtype=np.float32)
    by = np.uint8([[2], [1], [2], [1]])
    ap, summary, flag = twin.voc_ap(scores, by, np.int64([2]))
    assert ap[0] == 0.5 and summary.tolist() == [0.5, 1.0] and flag == 0
    assert helper.voc_ap(scores[:, 0].astype(np.float64), by[:, 0] == 2, np.arange(4), 2) == 0.5
    assert helper.voc_ap(scores[:, 0].astype(np.float64), by[:, 0] == 2, np.arange(4)[::-1].copy(), 2) == 0.5 * 1.0 + 0.5 * (2.0 / 3.0)
    det = ({"k,0001": [[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.1, 0.1], [0.5, 0.5, 1.0, 1.0], [0.0, 0.9, 0.1, 1.0]]},
           {"k,0001": [1, 1, 1, 1]}, {"k,0001": [0.25] * 4})
    gt = ({"k,0001": [[0.0, 0.0, 1.0, 1.0], [0.5, 0.5, 1.0, 1.0]]}, {"k,0001": [1, 1]}, {"k,0001": [1.0, 1.0]})
    m = helper.run_evaluation([{"id": 1, "name": "x"}], gt, det, set(), verbose=False)
    assert m[helper.MAP_KEY] == 0.5


def test_twin_flags_and_envelope():
    scores = np.float32([[0.9], [0.8], [0.7], [0.6], [0.5]])
    by = np.uint8([[1], [2], [1], [2], [2]])                    # p = 1/2, 2/4, 3/5: the envelope lifts the first two to 3/5
    ap, _, flag = twin.voc_ap(scores, by, np.int64([4]))
    assert flag == 0 and ap[0] == (0.25 * 0.6 + 0.25 * 0.6) + 0.25 * 0.6
    assert twin.voc_ap(scores, by, np.int64([4]), mutant="no_envelope")[0][0] < ap[0]
    ap, summary, flag = twin.voc_ap(scores, by, np.int64([2]))
    assert flag == twin.VOC_TP_ABOVE_GT and np.isnan(ap[0]) and np.isnan(summary[0]) and summary[1] == 0
    scores[1, 0] = np.inf
    assert twin.voc_ap(scores, by, np.int64([4]))[2] == twin.VOC_BAD_SCORE
    assert twin.voc_ap(scores[:0], by[:0], np.int64([3]))[0][0] == 0.0
    assert twin.voc_ap(np.float32([[0.5, 0.5]]), np.uint8([[2, 2]]), np.int64([1, 1]), total_gt=1)[2] == twin.VOC_GT_ABOVE_TOTAL


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(read):
    r, c = read["edge"], read["edge"]["c"]
    with pytest.raises(ValueError, match="1-indexed"):
        helper.run_evaluation([{"id": 0, "name": "z"}], ({}, {}, {}), ({}, {}, {}), set())
    gt = ({"k,0001": [[0.0, 0.0, 1.0, 1.0]]}, {"k,0001": [1]}, {"k,0001": [1.0]})
    two = ({"k,0001": [[0.0, 0.0, 1.0, 1.0]]}, {"k,0001": [2]}, {"k,0001": [0.5]})
    with pytest.raises(ValueError, match="outside"):
        helper.run_evaluation([{"id": 1, "name": "x"}], gt, two, set())
    nan = ({"k,0001": [[0.0, 0.0, 1.0, 1.0]]}, {"k,0001": [1]}, {"k,0001": [float("nan")]})
    with pytest.raises(ValueError, match="finite"):
        helper.run_evaluation([{"id": 1, "name": "x"}], gt, nan, set())
    with pytest.raises(ValueError, match="true positives"):
        helper.voc_ap(np.float64([0.5, 0.4]), np.array([True, True]), np.arange(2), 1)
    with pytest.raises(ValueError, match="evaluate_ava takes"):
        helper.evaluate_arrays(c["preds"][:, :3], c["boxes"], c["metadata"], r["excluded"], r["whitelist"], r["categories"],
                               r["groundtruth"], c["names"].tolist())
    from focus_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.voc_average_precision(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = torch.zeros(1, dtype=torch.int64)
        ops.ava_match(torch.zeros(1, 4), 3, torch.zeros(2, dtype=torch.int64), z, z, z, torch.zeros(0, dtype=torch.int32),
                      torch.zeros(0, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.uint8))


def test_config_and_module_surface():
    from focus_amd.slowfast import install_as_slowfast
    from focus_amd.slowfast.config.defaults import get_cfg
    a = get_cfg().AVA
    assert a.ANNOTATION_DIR == a.FRAME_DIR == a.FRAME_LIST_DIR == "" and a.FULL_TEST_ON_VAL is False
    assert a.TRAIN_LISTS == ["train.csv"] and a.TEST_LISTS == ["val.csv"] and a.GROUNDTRUTH_FILE == "ava_val_v2.2.csv"
    assert a.LABEL_MAP_FILE == "ava_action_list_v2.2_for_activitynet_2019.pbtxt"
    assert a.EXCLUSION_FILE == "ava_val_excluded_timestamps_v2.2.csv"
    install_as_slowfast()
    import slowfast.datasets.ava_helper as ah
    import slowfast.utils.ava_eval_helper as eh
    assert eh is helper and callable(ah.load_image_lists)
    for name in ("make_image_key", "read_csv", "read_exclusions", "read_labelmap", "get_ava_eval_data", "write_results",
                 "run_evaluation", "evaluate_ava"):
        assert callable(getattr(eh, name))
    assert issubclass(meters.DeviceAVAMeter, meters.AVAMeter)


def test_load_image_lists(read):
    from focus_amd.slowfast.datasets import ava_helper
    r, c = read["edge"], read["edge"]["c"]
    paths, names = ava_helper.load_image_lists(cases.make_cfg(r["root"]), False)
    assert names == c["names"].tolist() and len(paths) == len(names)
    assert paths[1] == [os.path.join("frames", "vidB/vidB_%06d.jpg" % i) for i in range(2)]


# ---- two ranks over gloo -----------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Model(torch.nn.Module):
    """A stand-in detector: the scores are looked up by the row numbers the loader put into meta."""

    def __init__(self, table):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.table = table

    def forward(self, x, meta, bboxes=None):
        return self.table[meta["row"].long()]


def _worker(rank, world, port, root, out):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from focus_amd import train
    from focus_amd.slowfast.utils import distributed as du
    got = du.all_gather_unaligned({"rank": rank, "pad": "x" * (1000 * rank), "t": torch.arange(rank + 2)})
    ok = [g["rank"] for g in got] == list(range(world)) and all(len(g["pad"]) == 1000 * i and g["t"].numel() == i + 2
                                                                 for i, g in enumerate(got))
    c = cases.case(cases.load(), "random")
    cfg = cases.make_cfg(root)
    cfg.DETECTION.ENABLE = True
    meter = meters.AVAMeter(1, cfg, "test")
    K = c["preds"].shape[0]
    chunks, o = [], 0                                           # unequal batches, dealt out in turn: rank 0 gets 40 rows where
    while o < K:                                                # rank 1 gets 25, and the gathered order is the original one
        n = 40 if len(chunks) % 2 == 0 else 25
        chunks.append(list(range(o, min(o + n, K))))
        o += n
    if len(chunks) % 2:
        chunks.append([])                                       # every rank makes the same number of gathers
    loader = []
    for rows in chunks[rank::2]:
        rows = torch.tensor(rows, dtype=torch.int64)
        loader.append((torch.zeros(1), None, None, {"boxes": torch.from_numpy(c["boxes"])[rows], "row": rows,
                                                    "ori_boxes": torch.from_numpy(c["boxes"])[rows],
                                                    "metadata": torch.from_numpy(c["metadata"])[rows]}))
    got_map = train.perform_test(loader, _Model(torch.from_numpy(c["preds"])), meter, cfg)
    if rank == 0:
        with open(out, "w") as f:
            f.write("%d %d %r" % (ok, sum(p.shape[0] for p in meter.all_preds), got_map))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gather_and_meter_over_gloo(read, tmp_path):
    import torch.multiprocessing as mp
    c = read["random"]["c"]
    out = str(tmp_path / "res.txt")
    mp.spawn(_worker, args=(2, _free_port(), read["random"]["root"], out), nprocs=2, join=True)
    ok, rows, got = open(out).read().split()
    assert ok == "1" and int(rows) == c["preds"].shape[0]
    bound = cases.check_ap(c, c["ap"], float(got), "two ranks")[1]
    assert abs(float(got) - float(c["map"])) <= bound
