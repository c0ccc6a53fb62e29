"""CPU: the n-body canonicalizer's routes off the device, its op-by-op path against the reference's fp64 vectors
(tests/golden/nbody_frame_grads.pt), and the three frame entry points in the header, the prototype table and ops."""
import os

import pytest
import torch

import nbody_frame_cases as fc
import equiadapt_amd as ea
from equiadapt_amd import _lib, ops

NEW_ENTRIES = ("eqa_nbody_frame_fwd", "eqa_nbody_frame_bwd", "eqa_rigid_rows_bwd")


def test_cpu_tensors_take_the_plain_routes():
    d = fc.inputs(5)
    can, _, _ = fc.golden_chain(ea.EuclideanGroupNBody, d, torch.float32)
    assert can.last_route.startswith("plain"), can.last_route
    assert can.last_invert_route.startswith("plain"), can.last_invert_route
    with torch.no_grad():
        fc.run(can, d["loc"], d["vel"])
        can.invert_canonicalization(d["loc"])
    assert can.last_route.startswith("plain") and can.last_invert_route.startswith("plain")
    assert list(can.canonicalization_info_dict["group_element"]) == ["rotation_matrix", "translation_vectors", "rotation_matrix_inverse"]


@pytest.mark.parametrize("M", fc.GOLDEN_SIZES)
def test_plain_path_equals_the_reference_in_fp64(golden, M):
    case = golden("nbody_frame_grads.pt")["cases"][M]
    d = fc.inputs(M)
    for k, stored in case["fp32"]["inputs"].items():
        assert torch.equal(d[k], stored), k                     # the helper still draws the inputs the file was made from
        assert torch.equal(stored.double(), case["fp64"]["inputs"][k]), k
    _, out, grads = fc.golden_chain(ea.EuclideanGroupNBody, d, torch.float64)
    for k, ref in case["fp64"]["outputs"].items():
        assert out[k].dtype == torch.float64 and (out[k] - ref.reshape(out[k].shape)).abs().max() <= 1e-12, k
    for k, ref in case["fp64"]["grads"].items():
        assert (grads[k] - ref).abs().max() <= 1e-12, k


def test_header_and_prototype_table_name_the_new_entries():
    with open(os.path.join(_lib.INCLUDE, "eqa_hip.h")) as f:
        header = f.read()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    assert len(_lib.SIGNATURES["eqa_nbody_frame_fwd"][1]) == 9
    assert len(_lib.SIGNATURES["eqa_nbody_frame_bwd"][1]) == 14
    assert len(_lib.SIGNATURES["eqa_rigid_rows_bwd"][1]) == 7


def test_ops_reject_wrong_shapes():
    v, r = torch.zeros(4, 3, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError):
        ops.nbody_frame_fwd(torch.zeros(4, 9), r, r, r)
    with pytest.raises(ValueError):
        ops.nbody_frame_fwd(v, torch.zeros(5, 3), r, r)
    with pytest.raises(ValueError):
        ops.nbody_frame_fwd(v, r, r, torch.zeros(4, 4))
    with pytest.raises(ValueError):
        ops.nbody_frame_bwd(torch.zeros(4, 3), r, r, r, v, v, r, r)
    with pytest.raises(ValueError):
        ops.nbody_frame_bwd(v, r, r, r, v, torch.zeros(4, 3), r, r)
    with pytest.raises(ValueError):
        ops.nbody_frame_bwd(v, r, r, r, v, v, torch.zeros(3, 3), r)
    with pytest.raises(ValueError):
        ops.nbody_frame_bwd(v, r, r, r, None, v, r, r)                                  # gt, gloc, gvel need R
    with pytest.raises(ValueError):
        ops.nbody_frame_bwd(v, None, None, None, None, v, None, None, need=(False,) * 4)
    with pytest.raises(ValueError):
        ops.rigid_rows_bwd(r, v, torch.zeros(4, 3, 3))
    with pytest.raises(ValueError):
        ops.rigid_rows_bwd(torch.zeros(5, 3), v, r)
    with pytest.raises(ValueError):
        ops.rigid_rows_bwd(r, torch.zeros(4, 9), r)
