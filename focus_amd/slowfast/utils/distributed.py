"""torch.distributed helpers the train step uses (mirror of the hot subset of slowfast/utils/distributed.py)."""
import torch
import torch.distributed as dist

_LOCAL_PROCESS_GROUP = None


def get_world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def get_rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def is_master_proc(num_gpus=8):
    return get_rank() % num_gpus == 0 if dist.is_initialized() else True


def is_root_proc():
    return get_rank() == 0 if dist.is_initialized() else True


def all_gather(tensors):
    """distributed.py:15-34: gather along dim 0 from every rank."""
    world = get_world_size()
    if world == 1:
        return list(tensors)
    out = []
    for t in tensors:
        parts = [torch.ones_like(t) for _ in range(world)]
        dist.all_gather(parts, t, async_op=False)
        out.append(torch.cat(parts, dim=0))
    return out


def all_reduce(tensors, average=True):
    """distributed.py:37-53 issues one blocking all-reduce per scalar; here the scalars are packed into one
    buffer and reduced with a single collective."""
    if get_world_size() == 1:
        return tensors
    flat = torch.stack([t.detach().float().reshape(()) for t in tensors])
    dist.all_reduce(flat)
    if average:
        flat = flat / get_world_size()
    return [flat[i].to(t.dtype) for i, t in enumerate(tensors)]


_GLOO_GROUP = None


def _global_gloo_group():
    """All ranks over gloo: the world itself when it is a gloo world, else a side group made once."""
    global _GLOO_GROUP
    if dist.get_backend() == "gloo":
        return dist.group.WORLD
    if _GLOO_GROUP is None:
        _GLOO_GROUP = dist.new_group(backend="gloo")
    return _GLOO_GROUP


def all_gather_unaligned(data, group=None):
    """distributed.py:229-265: all-gather of any picklable object, one per rank and of any size -> the list of the ranks'
    objects in rank order.  The pickles travel as byte tensors over a gloo group (on the host), padded to the longest; the
    lengths are gathered first."""
    import pickle
    if get_world_size() == 1:
        return [data]
    if group is None:
        group = _global_gloo_group()
    world = dist.get_world_size(group)
    if world == 1:
        return [data]
    device = torch.device("cpu" if dist.get_backend(group) == "gloo" else "cuda")
    payload = torch.frombuffer(bytearray(pickle.dumps(data)), dtype=torch.uint8).to(device)
    sizes = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([payload.numel()], dtype=torch.int64, device=device), group=group)
    sizes = [int(s.item()) for s in sizes]
    padded = torch.zeros(max(sizes), dtype=torch.uint8, device=device)
    padded[:payload.numel()] = payload
    parts = [torch.empty_like(padded) for _ in sizes]
    dist.all_gather(parts, padded, group=group)
    return [pickle.loads(p.cpu().numpy().tobytes()[:n]) for n, p in zip(sizes, parts)]


def init_distributed_training(cfg):
    """distributed.py:268-285: one process group per machine (the ranks that share xGMI)."""
    global _LOCAL_PROCESS_GROUP
    if cfg.NUM_GPUS <= 1 or not (dist.is_available() and dist.is_initialized()):
        return
    per = cfg.NUM_GPUS
    for i in range(dist.get_world_size() // per):
        pg = dist.new_group(list(range(i * per, (i + 1) * per)))
        if i == cfg.SHARD_ID:
            _LOCAL_PROCESS_GROUP = pg


def get_local_size():
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group=_LOCAL_PROCESS_GROUP)


def get_local_rank():
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    assert _LOCAL_PROCESS_GROUP is not None
    return dist.get_rank(group=_LOCAL_PROCESS_GROUP)


def synchronize():
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()
