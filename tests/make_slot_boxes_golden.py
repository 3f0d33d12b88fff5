"""TEST INFRASTRUCTURE: writes tests/golden/slot_boxes.npz from the reference's own slowfast/utils/box_ops.py, loaded as a
single file (its module-level imports of torchvision and scipy are satisfied by stubs where the packages are absent:
masks_to_boxes calls neither).  Runs only where the reference tree is present:
    python tests/make_slot_boxes_golden.py
The fixture is data only.  Per case of slot_seg_ref.CASES: a small fp32 slot-attention tensor attn [B,T,N,K]; the arg-max
map of the masks as STEVE hands them out (transposed to [B,T,K,He,We], nearest-upsampled by repeat_interleave, torch.argmax
over the slot axis), sampled back at one pixel per cell after checking that it is constant over every cell; and the
reference's masks_to_boxes of the upsampled one-hot masks, [B,T,K,4].  Seeds are searched so that every slot owns a cell in
every frame: the reference's value for an empty mask is not part of the contract."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import slot_seg_ref  # noqa: E402


def _stub(name, **attrs):
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        full = ".".join(parts[:i])
        if full not in sys.modules:
            sys.modules[full] = types.ModuleType(full)
        if i > 1:
            setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], sys.modules[full])
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def load_reference():
    from oracle._ref_loader import REF

    def absent(*a, **k):
        raise RuntimeError("stub: not used by masks_to_boxes")
    try:
        import torchvision.ops.boxes  # noqa: F401
    except ImportError:
        _stub("torchvision.ops.boxes", box_area=absent)
    try:
        import scipy.optimize  # noqa: F401
    except ImportError:
        _stub("scipy.optimize", linear_sum_assignment=absent)
    spec = importlib.util.spec_from_file_location("_reference_box_ops", os.path.join(REF, "slowfast", "utils", "box_ops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(ref, attn, He, We, sy, sx):
    """-> (seg uint8 [B,T,N], boxes fp32 [B,T,K,4]) by the reference's route, or None if a slot is empty in some frame."""
    B, T, N, K = attn.shape
    a = torch.from_numpy(attn).transpose(-1, -2).reshape(B, T, K, He, We)
    a = a.repeat_interleave(sy, dim=-2).repeat_interleave(sx, dim=-1)                     # B, T, K, H, W
    am = torch.argmax(a, dim=2)                                                           # B, T, H, W
    cells = am[:, :, ::sy, ::sx]
    assert torch.equal(cells.repeat_interleave(sy, dim=-2).repeat_interleave(sx, dim=-1), am)
    onehot = torch.zeros_like(a).scatter_(2, am.unsqueeze(2), 1.0)
    if not bool(onehot.flatten(3).sum(-1).gt(0).all()):
        return None
    boxes = ref.masks_to_boxes(onehot.flatten(end_dim=2))
    assert boxes.dtype == torch.float32
    return cells.reshape(B, T, N).to(torch.uint8).numpy(), boxes.reshape(B, T, K, 4).numpy()


def main():
    ref = load_reference()
    out = {}
    for tag, (B, T, He, We, K, sy, sx, levels) in slot_seg_ref.CASES.items():
        for seed in range(100000):
            attn = slot_seg_ref.thin_attn() if tag == "thin" else slot_seg_ref.make_attn(B, T, He, We, K, seed, levels)
            got = record(ref, attn, He, We, sy, sx)
            if got is not None and (not levels or has_ties(attn)):
                break
            assert tag != "thin"
        else:
            raise RuntimeError("no seed found for " + tag)
        out.update({tag + ".seed": np.int64(seed), tag + ".attn": attn, tag + ".seg": got[0], tag + ".boxes": got[1]})
        print(tag, "seed", seed, attn.shape, "bytes", attn.nbytes)
    np.savez_compressed(slot_seg_ref.GOLDEN, **out)
    print("wrote", slot_seg_ref.GOLDEN, os.path.getsize(slot_seg_ref.GOLDEN), "bytes")


def has_ties(attn):
    """Some cell whose maximum is reached by more than one slot: the case is about the tie rule."""
    return bool(((attn == attn.max(-1, keepdims=True)).sum(-1) > 1).any())


if __name__ == "__main__":
    main()
