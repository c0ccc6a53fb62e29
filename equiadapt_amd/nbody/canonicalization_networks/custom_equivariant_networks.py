"""VNDeepSets: the vector-neuron deep-sets network that predicts the E(3) frame of an n-body system.

Reference: equiadapt/nbody/canonicalization_networks/custom_equivariant_networks.py:13-281 (``VNDeepSets``, ``VNDeepSetLayer``,
``SequentialMultiple``).  Same constructor, attributes, ``forward(nodes, loc, edges, vel, edge_attr, charges)`` and
``state_dict()`` keys and shapes, so a reference checkpoint loads by key.  The reference's one dependency outside torch,
``torch_scatter.scatter(..., reduce="sum" | "mean")``, is restated as an index-add (``_scatter``).

Two routes compute the same function:

* the plain route: torch ops as the reference has them; any device, any dtype, any graph, with autograd through everything;
* the fused route (fp32 on the device): ``eqa_vndeepsets_fwd`` evaluates the whole network in one launch, and
  ``eqa_vndeepsets_train_fwd`` / ``eqa_vndeepsets_bwd`` train it (gradients for the parameters; csrc/nbody.hip), compiled for hidden widths 8, 16 and 32: another hidden_dim is
  zero-padded to the next one, which is exact.  It takes the
  graph as per-system in-edge counts, which ``eqa_nbody_adjacency`` builds and validates once per distinct ``edges`` pair
  (nbody/graph.py).  ``EQA_NBODY_KERNEL=0`` forces the plain route.  ``last_route`` records which one the last call took.
"""
import os
import types
from typing import Any, List, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from equiadapt_amd import ops
from equiadapt_amd.nbody import graph
from equiadapt_amd.nbody.canonicalization_networks.custom_group_equivariant_layers import VNLeakyReLU, VNSoftplus

_NBODY_KERNEL = "EQA_NBODY_KERNEL"      # "0": the plain route on the device as well (A/B timing: tools/kbench_nbody.py)
_CANON_FEATURES = ("p", "pv", "pva", "pvc", "pvac")


def _scatter(src: torch.Tensor, index: torch.Tensor, reduce: str) -> torch.Tensor:
    """``torch_scatter.scatter(src, index, 0, reduce=reduce)`` for sum / mean: an index-add into ``index.max() + 1`` rows; the
    mean divides by the number of contributions, clamped to 1 (a row nothing was added to stays 0)."""
    if reduce not in ("sum", "mean"):
        raise NotImplementedError(f"pooling '{reduce}' is not restated here: only 'sum' and 'mean' are")
    rows = int(index.max()) + 1
    out = src.new_zeros((rows,) + tuple(src.shape[1:])).index_add_(0, index, src)
    if reduce == "mean":
        count = src.new_zeros(rows).index_add_(0, index, src.new_ones(index.shape[0])).clamp_(min=1)
        out = out / count.view((rows,) + (1,) * (src.dim() - 1))
    return out


class VNDeepSets(nn.Module):
    """
    Args:
        hyperparams: an object read by attribute (or a dict): ``hidden_dim, num_layers, nonlinearity ("relu" | "leakyrelu" |
            "softplus"), canon_feature ("p" | "pv" | "pva" | "pvc" | "pvac"), canon_translation, angular_feature, layer_pooling,
            final_pooling ("sum" | "mean"), dropout, out_dim, batch_size``; optional ``learning_rate, weight_decay, patience``.
        device: where ``dummy_input`` / ``dummy_indices`` live (the reference's default: "cuda" if available).

    As in the reference, a system has 5 bodies and ``loc`` holds ``5 * batch_size`` nodes (anything else is a ``ValueError``).
    ``out_dim == 1`` is prediction mode: the squeezed per-node output of the output layer.  Otherwise the result is
    ``(rotation_vectors (M, 3, 3), translation_vectors (M, 3))``, constant over a system's bodies.

    The layers are ``nn.Linear`` WITH bias on the channel axis of ``(M, 3, C)`` features, as the reference has them.  A bias adds
    the same constant to all three spatial components, which no rotation leaves in place: the network is rotation equivariant
    only while its biases are zero (translation equivariance and permutation invariance hold regardless).  Kept, not repaired.
    """

    def __init__(self, hyperparams: Any, device: str = "cuda" if torch.cuda.is_available() else "cpu") -> None:
        super().__init__()
        if isinstance(hyperparams, dict):
            hyperparams = types.SimpleNamespace(**hyperparams)
        self.device: str = device
        self.learning_rate = hyperparams.learning_rate if hasattr(hyperparams, "learning_rate") else None
        self.weight_decay = hyperparams.weight_decay if hasattr(hyperparams, "weight_decay") else 0.0
        self.patience = hyperparams.patience if hasattr(hyperparams, "patience") else 100
        self.prediction_mode: bool = hyperparams.out_dim == 1
        self.model: str = "vndeepsets"
        self.hidden_dim: int = hyperparams.hidden_dim
        self.layer_pooling: str = hyperparams.layer_pooling
        self.final_pooling: str = hyperparams.final_pooling
        self.num_layers: int = hyperparams.num_layers
        self.nonlinearity: str = hyperparams.nonlinearity
        self.canon_feature: str = hyperparams.canon_feature
        self.canon_translation: bool = hyperparams.canon_translation
        self.angular_feature: bool = hyperparams.angular_feature
        self.dropout: float = hyperparams.dropout
        self.out_dim: int = hyperparams.out_dim
        self.in_dim: int = len(self.canon_feature)
        self.first_set_layer = VNDeepSetLayer(self.in_dim, self.hidden_dim, self.nonlinearity, self.layer_pooling, False,
                                              dropout=self.dropout)
        self.set_layers = SequentialMultiple(*[
            VNDeepSetLayer(self.hidden_dim, self.hidden_dim, self.nonlinearity, self.layer_pooling, dropout=self.dropout)
            for _ in range(self.num_layers - 1)])
        self.output_layer = nn.Linear(self.hidden_dim, self.out_dim)
        self.batch_size: int = hyperparams.batch_size

        self.dummy_input: torch.Tensor = torch.zeros(1, device=self.device, dtype=torch.long)
        self.dummy_indices: torch.Tensor = torch.zeros(1, device=self.device, dtype=torch.long)
        self._padding_index_cache: dict = {}       # (width, device) -> (index, padded length): see _padding_index
        self.last_route: Optional[str] = None      # "fused-inference" | "fused-train" | "plain: <why>"

    # ------------------------------------------------------------------------------------------------------------------ routes
    def forward(self, nodes: torch.Tensor, loc: torch.Tensor, edges: Union[torch.Tensor, List[torch.Tensor]], vel: torch.Tensor,
                edge_attr: torch.Tensor, charges: torch.Tensor, _dropout_mask: Optional[torch.Tensor] = None
                ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """``_dropout_mask`` (private; tests and A/B runs): the step's dropout factors ``(num_layers, M, 3, hidden_dim)``, already
        scaled by ``1 / (1 - p)``, used by either route in place of a draw of its own."""
        if loc.shape[0] != 5 * self.batch_size:
            raise ValueError(f"VNDeepSets was built for batch_size = {self.batch_size} systems of 5 bodies = {5 * self.batch_size} "
                             f"nodes; loc has {loc.shape[0]} (the reference fails inside torch_scatter here)")
        why = self._plain_reason(loc, edges, vel, charges)
        if why is None:
            return self._fused_forward(loc, edges, vel, charges, _dropout_mask)
        self.last_route = "plain: " + why
        return self._plain_forward(loc, edges, vel, charges, _dropout_mask)

    def _plain_forward(self, loc, edges, vel, charges, dropout_mask):
        batch_indices = torch.arange(self.batch_size, device=loc.device).reshape(-1, 1).repeat(1, 5).reshape(-1)
        mean_loc = _scatter(loc, batch_indices, self.layer_pooling)
        mean_loc = mean_loc.repeat(5, 1, 1).transpose(0, 1).reshape(-1, 3)
        canonical_loc = loc - mean_loc

        if self.canon_feature == "p":
            features = torch.stack([canonical_loc], dim=2)
        if self.canon_feature == "pv":
            features = torch.stack([canonical_loc, vel], dim=2)
        elif self.canon_feature == "pva":
            angular = torch.linalg.cross(canonical_loc, vel, dim=1)
            features = torch.stack([canonical_loc, vel, angular], dim=2)
        elif self.canon_feature == "pvc":
            features = torch.stack([canonical_loc, vel, canonical_loc * charges], dim=2)
        elif self.canon_feature == "pvac":
            angular = torch.linalg.cross(canonical_loc, vel, dim=1)
            features = torch.stack([canonical_loc, vel, angular, canonical_loc * charges], dim=2)

        masks = [None] * self.num_layers if dropout_mask is None else list(dropout_mask)
        x, _ = self.first_set_layer(features, edges, masks[0])
        for layer, mask in zip(self.set_layers, masks[1:]):
            x, _ = layer(x, edges, mask)

        if self.prediction_mode:
            return self.output_layer(x).squeeze()
        x = _scatter(x, batch_indices, self.final_pooling)
        output = self.output_layer(x)
        output = output.repeat(5, 1, 1, 1).transpose(0, 1).reshape(-1, 3, 4)

        rotation_vectors = output[:, :, :3]
        translation_vectors = output[:, :, 3:] if self.canon_translation else 0.0
        translation_vectors = translation_vectors + mean_loc[:, :, None]
        return rotation_vectors, translation_vectors.squeeze()

    def _plain_reason(self, loc, edges, vel, charges) -> Optional[str]:
        """None when the fused route applies; else why not (everything but the edges' validity, which `_fused_forward` asks)."""
        if os.environ.get(_NBODY_KERNEL, "1") == "0":
            return f"{_NBODY_KERNEL}=0"
        if self.prediction_mode or self.out_dim != 4:
            return "prediction mode" if self.prediction_mode else f"out_dim = {self.out_dim}"
        if not (1 <= self.hidden_dim <= ops.VNDEEPSETS_MAX_HIDDEN and 1 <= self.num_layers <= ops.VNDEEPSETS_MAX_LAYERS):
            return f"hidden_dim = {self.hidden_dim}, num_layers = {self.num_layers} beyond the kernels' limits"
        if self.layer_pooling not in ("sum", "mean") or self.final_pooling not in ("sum", "mean"):
            return "pooling"
        if self.canon_feature not in _CANON_FEATURES or self.nonlinearity not in ("relu", "leakyrelu", "softplus"):
            return "feature string or nonlinearity the kernels do not know"
        used = [loc] + ([vel] if "v" in self.canon_feature else []) + ([charges] if "c" in self.canon_feature else [])
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in used):
            return "inputs are not fp32 device tensors"
        if not all(p.is_cuda and p.dtype == torch.float32 and p.device == loc.device for p in self.parameters()):
            return "parameters are not fp32 on the inputs' device"
        grad = torch.is_grad_enabled()
        if grad and any(t.requires_grad for t in used):
            return "an input requires grad"
        if grad and self.nonlinearity == "softplus" and any(p.requires_grad for p in self.parameters()):
            return "softplus under autograd"
        if any(m.nonlinear_function.map_to_dir.weight.shape[0] != self.hidden_dim for m in self._layers()):
            return "share_nonlinearity"
        rows, cols = edges[0], edges[1]
        if not all(isinstance(e, torch.Tensor) and e.dtype == torch.int64 and e.device == loc.device and e.dim() == 1
                   and e.is_contiguous() for e in (rows, cols)) or rows.numel() != cols.numel() or rows.numel() == 0:
            return "edges are not two int64 index vectors on the inputs' device"
        return None

    def _layers(self):
        return [self.first_set_layer, *self.set_layers]

    def _padded_width(self) -> int:
        return next(w for w in ops.VNDEEPSETS_WIDTHS if w >= self.hidden_dim)

    def _padding_index(self, width: int, device) -> torch.Tensor:
        """Where each packed parameter goes in the packing of the same network at hidden_dim = `width` (the kernels' compiled
        widths).  The added channels have zero weights and biases, so they stay exactly zero through every layer."""
        key = (width, str(device))
        cache = self._padding_index_cache
        if key not in cache:
            index, offset = [], 0
            for p in self.parameters():
                real = tuple(p.shape) if p.dim() == 2 else (1, p.shape[0])
                first = p is self.first_set_layer.identity_linear.weight or p is self.first_set_layer.pooling_linear.weight
                if p is self.output_layer.bias:
                    padded = real                                   # (4)
                elif p is self.output_layer.weight:
                    padded = (real[0], width)                       # (4, H)
                elif p.dim() == 1:
                    padded = (1, width)                             # (H)
                else:
                    padded = (width, real[1] if first else width)   # (H, in_dim): in_dim is not padded; (H, H)
                rows, cols = torch.arange(real[0])[:, None], torch.arange(real[1])[None, :]
                index.append((rows * padded[1] + cols).reshape(-1) + offset)
                offset += padded[0] * padded[1]
            cache[key] = (torch.cat(index).to(device), offset)
        return cache[key]

    def _kernel_config(self) -> dict:
        f = self.canon_feature
        return dict(hidden=self._padded_width(), layers=self.num_layers,
                    features=(1 if "v" in f else 0) | (2 if "a" in f else 0) | (4 if "c" in f else 0),
                    softplus=self.nonlinearity == "softplus",
                    slope=float(self._layers()[0].nonlinear_function.negative_slope),
                    layer_mean=self.layer_pooling == "mean", final_mean=self.final_pooling == "mean",
                    canon_translation=bool(self.canon_translation))

    def _fused_forward(self, loc, edges, vel, charges, dropout_mask):
        ok, adj = graph.adjacency_cache.lookup(edges[0], edges[1], self.batch_size)
        if not ok:
            self.last_route = "plain: edges leave a system, are out of range or give the last node no incoming edge"
            return self._plain_forward(loc, edges, vel, charges, dropout_mask)
        cfg = self._kernel_config()
        vel = vel if "v" in self.canon_feature else None
        charges = charges if "c" in self.canon_feature else None
        M = loc.shape[0]
        if dropout_mask is None and self.training and self.dropout > 0:
            keep = 1.0 - self.dropout
            dropout_mask = (torch.rand(self.num_layers, M, 3, self.hidden_dim, device=loc.device) < keep).to(torch.float32)
            if keep > 0:
                dropout_mask = dropout_mask / keep
        packed = torch.cat([p.reshape(-1) for p in self.parameters()])     # the one differentiable input of the fused route
        width = cfg["hidden"]
        if width != self.hidden_dim:
            index, length = self._padding_index(width, loc.device)
            packed = packed.new_zeros(length).index_copy(0, index, packed)
            if dropout_mask is not None:
                dropout_mask = torch.nn.functional.pad(dropout_mask, (0, width - self.hidden_dim))
        if packed.requires_grad or dropout_mask is not None:
            self.last_route = "fused-train"
            return _VNDeepSetsFunction.apply(packed, loc, vel, charges, adj, dropout_mask, cfg)
        self.last_route = "fused-inference"
        return ops.vndeepsets_fwd(loc, vel, charges, adj, packed, **cfg)


class _VNDeepSetsFunction(torch.autograd.Function):
    """(rotation_vectors, translation_vectors) as a function of the packed parameters; the inputs get no gradient (a call whose
    inputs require one takes the plain route)."""

    @staticmethod
    def forward(ctx, packed, loc, vel, charges, adj, mask, cfg):
        rot, trans, saved = ops.vndeepsets_train_fwd(loc, vel, charges, adj, packed, mask, **cfg)
        ctx.save_for_backward(packed, loc, vel, charges, adj, mask, saved)
        ctx.cfg = cfg
        return rot, trans

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_rot, grad_trans):
        packed, loc, vel, charges, adj, mask, saved = ctx.saved_tensors
        partial = ops.vndeepsets_bwd(loc, vel, charges, adj, packed, mask, saved, grad_rot, grad_trans, **ctx.cfg)
        return partial.sum(0), None, None, None, None, None, None


class VNDeepSetLayer(nn.Module):
    """identity_linear(x) + pooling_linear(pool of x over each node's incoming edges), the vector nonlinearity, dropout and, but
    for the first layer, a residual.  ``x``: (M, 3, C); ``edges``: rows (sources) and cols (targets)."""

    def __init__(self, in_channels: int, out_channels: int, nonlinearity: str, pooling: str = "sum", residual: bool = True,
                 dropout: float = 0.0):
        super().__init__()
        self.in_dim: int = in_channels
        self.out_dim: int = out_channels
        self.pooling: str = pooling
        self.residual: bool = residual
        self.nonlinearity: str = nonlinearity
        self.dropout: float = dropout

        self.identity_linear = nn.Linear(in_channels, out_channels)
        self.pooling_linear = nn.Linear(in_channels, out_channels)
        self.dropout_layer = nn.Dropout(self.dropout)

        if self.nonlinearity == "softplus":
            self.nonlinear_function = VNSoftplus(out_channels, share_nonlinearity=False)
        elif self.nonlinearity == "relu":
            self.nonlinear_function = VNLeakyReLU(out_channels, share_nonlinearity=False, negative_slope=0.0)
        elif self.nonlinearity == "leakyrelu":
            self.nonlinear_function = VNLeakyReLU(out_channels, share_nonlinearity=False)

    def forward(self, x: torch.Tensor, edges: Union[torch.Tensor, List[torch.Tensor]], _dropout_mask: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, Any]:
        edges_1 = edges[0]
        edges_2 = edges[1]

        identity = self.identity_linear(x)

        nodes_1 = torch.index_select(x, 0, edges_1)
        pooled_set = _scatter(nodes_1, edges_2, self.pooling)
        pooling = self.pooling_linear(pooled_set)

        output = self.nonlinear_function((identity + pooling).transpose(1, -1)).transpose(1, -1)

        output = self.dropout_layer(output) if _dropout_mask is None else output * _dropout_mask

        if self.residual:
            output = output + x

        return output, edges


class SequentialMultiple(nn.Sequential):
    """``nn.Sequential`` whose modules take and return several values (a tuple is passed on unpacked)."""

    def forward(self, *inputs: torch.Tensor) -> torch.Tensor:
        for module in self._modules.values():
            if type(inputs) is tuple:
                inputs = module(*inputs)
            else:
                inputs = module(inputs)
        return inputs
