"""One process per GPU. Environments shard by global id (lnw.shard); the step
has no collective. Collectives are used only off the step path: the bench's
max-over-ranks wall time and optional episode-counter sums (RCCL all_reduce
over xGMI on the GPU box, gloo on CPU), and the two exchanges of a minibatch
drawn over sharded rollouts (all_gather, all_reduce_sum_: lnw.ppodist)."""
import os

import torch
import torch.distributed as dist

from .shard import env_range  # noqa: F401


def world():
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), \
        int(os.environ.get("LOCAL_RANK", "0"))


def launched():
    """True under a launcher (torch.distributed.run sets TORCHELASTIC_RUN_ID)."""
    return "TORCHELASTIC_RUN_ID" in os.environ


def init(backend=None):
    """Initialise the default process group when launched with WORLD_SIZE > 1,
    or under torch.distributed.run with one rank (the RCCL path then runs with
    a world of one). Returns (world_size, rank, local_rank)."""
    ws, rank, local = world()
    if (ws > 1 or launched()) and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        kw = {}
        if backend == "nccl":
            kw["device_id"] = torch.device("cuda", local)
        dist.init_process_group(backend, **kw)
    return ws, rank, local


def backend():
    """The process group's backend ("nccl" = RCCL on ROCm, "gloo"), or None."""
    return dist.get_backend() if dist.is_initialized() else None


def size():
    """The rank count the process group (RCCL / gloo) reports, or None."""
    return dist.get_world_size() if dist.is_initialized() else None


def _dev():
    return torch.device("cuda", torch.cuda.current_device()) if (
        dist.is_initialized() and dist.get_backend() == "nccl") else torch.device("cpu")


def reduce_max(values):
    """Element-wise max over ranks of a list of floats (the slowest rank's time)."""
    t = torch.tensor(values, dtype=torch.float64, device=_dev())
    if dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return [float(v) for v in t.cpu()]


def reduce_sum(values):
    t = torch.tensor(values, dtype=torch.float64, device=_dev())
    if dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return [float(v) for v in t.cpu()]


def _staged(group):
    """True when a collective on a device tensor has to go through the host
    (gloo); RCCL takes the device tensor on the current stream."""
    return dist.get_backend(group) != "nccl"


def all_gather(t, group=None):
    """Every rank's copy of the 1-d tensor `t`, as [world, t.numel()] on t's
    device, rank order. "nccl": on the device tensors, on the current stream,
    nothing synchronises with the host; "gloo": staged through the host (it
    synchronises). No process group: t[None], a world of one."""
    if not dist.is_initialized():
        return t[None]
    ws = dist.get_world_size(group)
    if t.is_cuda and _staged(group):
        host = t.cpu()
        out = torch.empty(ws * host.numel(), dtype=host.dtype)
        dist.all_gather_into_tensor(out, host, group=group)
        return out.to(t.device).view(ws, -1)
    out = torch.empty(ws * t.numel(), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t, group=group)
    return out.view(ws, -1)


def all_reduce_sum_(t, group=None):
    """Element-wise sum over ranks, in place, of a tensor of any dtype the
    backend sums (int32 for lnw.ppodist's exchange buffer); staged as
    all_gather is. Returns t."""
    if not dist.is_initialized():
        return t
    if t.is_cuda and _staged(group):
        host = t.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        t.copy_(host)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def rank_size(group=None):
    """(rank, world size) in `group`, (0, 1) with no process group."""
    if not dist.is_initialized():
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


def barrier():
    if dist.is_initialized():
        dist.barrier()


def finalize():
    if dist.is_initialized():
        dist.destroy_process_group()
