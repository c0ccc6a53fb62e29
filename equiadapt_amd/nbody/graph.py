"""Edge lists of batched n-body systems: the complete graph the reference's example builds, and the validated per-system
adjacency the fused VNDeepSets kernels take instead of the two index vectors."""
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from equiadapt_amd import ops

BODIES = 5     # bodies per system: hard-wired in the reference network (``repeat(1, 5)``)

_COMPLETE_CAPACITY = 8
_complete: "OrderedDict[tuple, List[torch.Tensor]]" = OrderedDict()


def complete_graph_edges(batch_size: int, n_nodes: int = BODIES, device="cpu") -> List[torch.Tensor]:
    """``[rows, cols]`` of examples/nbody/model_utils.get_edges: every ordered pair i != j of each system's ``n_nodes`` nodes,
    system b offset by ``b * n_nodes``, i outermost.  Built once per (batch_size, n_nodes, device) and kept for the 8 keys used most
    recently: every call returns the same two tensors, so a loop that takes its edges from here validates them for the fused
    route once.  The pair is shared by all callers and must not be modified in place."""
    if batch_size < 1:
        raise ValueError("Batch size must be greater than or equal to 1.")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(batch_size), int(n_nodes), device)
    hit = _complete.get(key)
    if hit is not None:
        _complete.move_to_end(key)
        return hit
    i, j = torch.meshgrid(torch.arange(n_nodes), torch.arange(n_nodes), indexing="ij")
    keep = i != j
    offset = (torch.arange(batch_size) * n_nodes)[:, None]
    rows = (i[keep][None, :] + offset).reshape(-1).to(device)
    cols = (j[keep][None, :] + offset).reshape(-1).to(device)
    hit = _complete[key] = [rows, cols]
    while len(_complete) > _COMPLETE_CAPACITY:
        _complete.popitem(last=False)
    return hit


class AdjacencyCache:
    """Verdict and in-edge counts of an ``edges`` pair, keyed by (data_ptr, numel, _version) of both tensors, the device and the number of systems.
    An entry holds the two tensors, so their memory cannot be handed to other tensors while the entry lives; ``flag_reads``
    counts the 4-byte device-to-host copies (one per miss)."""

    def __init__(self, capacity: int = 8) -> None:
        self.capacity = capacity
        self.entries: "OrderedDict[tuple, tuple]" = OrderedDict()
        self.flag_reads = 0

    def lookup(self, rows: torch.Tensor, cols: torch.Tensor, systems: int) -> Tuple[bool, Optional[torch.Tensor]]:
        key = (rows.data_ptr(), rows.numel(), rows._version, cols.data_ptr(), cols.numel(), cols._version, systems, rows.device)
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            return hit[0], hit[1]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("VNDeepSets: these edges have not been validated yet, and validation reads a flag back from the "
                               "device, which a hipGraph capture cannot hold.  Run one forward with the same edge tensors "
                               "(nbody.complete_graph_edges returns the same pair every call) before capturing.")
        adj, flag = ops.nbody_adjacency(rows, cols, systems)
        self.flag_reads += 1
        ok = int(flag.item()) == ops.NBODY_EDGES_OK
        self.entries[key] = (ok, adj if ok else None, rows, cols)
        while len(self.entries) > self.capacity:
            self.entries.popitem(last=False)
        return ok, (adj if ok else None)


adjacency_cache = AdjacencyCache()
