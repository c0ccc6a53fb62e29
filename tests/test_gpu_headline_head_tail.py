"""The headline step with its head (crop + resize writing pixels and the lifting kernel's bound: eqa_crop_resize_aa_nhwc) and its tail
(eqa_window_sums_tail on the inverse transform's partials) against the launches they replace (`EQA_HEAD_FUSED=0`, `EQA_TAIL_FUSED=0`:
planar resize, layout copy, eqa_absmax_slots; finalize, GEMV, argmax, table lookups): every output of the step bit for bit.

The network is bench.py's (32 fields, C8, k = 5, three layers) on 224 x 224 images, at B = 2 and B = 5: two and five images are fewer
tiles than `fftconv.MIN_TILES` sends through the FFT route, so the test lowers that knob -- the launches are the headline's, on fewer
images (B = 5: an odd count, blocks of the resize kernel without an image, tiles of the last image behind a padding row)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def can(dev):
    import bench

    return bench.build_canonicalizer(dev)


def _step(can, x, f, monkeypatch, fused: bool):
    from equiadapt_amd.images.canonicalization_networks import fftconv

    monkeypatch.setattr(fftconv, "MIN_TILES", 1)
    monkeypatch.setenv("EQA_HEAD_FUSED", "1" if fused else "0")
    monkeypatch.setenv("EQA_TAIL_FUSED", "1" if fused else "0")
    with torch.no_grad():
        y = can(x)
        inv = can.invert_canonicalization(f, induced_rep_type="scalar")
    info = can.canonicalization_info_dict
    return {"activations": info["group_activations"], "index": info["group_index"], "argmax_index": info["argmax_index"],
            "rotation": info["group_element"]["rotation"], "canonicalized": y, "inverted": inv,
            "routes": list(can.canonicalization_network.last_routes)}


@pytest.mark.parametrize("B", [2, 5])
def test_both_switches_on_and_off_give_the_same_step(dev, can, monkeypatch, B):
    g = torch.Generator().manual_seed(B)
    x, f = torch.randn(B, 3, 224, 224, generator=g).to(dev), torch.randn(B, 3, 224, 224, generator=g).to(dev)
    old = _step(can, x, f, monkeypatch, False)
    new = _step(can, x, f, monkeypatch, True)
    assert old["routes"] == ["lift_fused", "fft5", "bound:eqa_absmax_slots", "tail:finalize+eqa_window_sums_gemv"], old["routes"]
    assert new["routes"] == ["lift_fused", "fft5", "bound:crop_slots", "tail:eqa_window_sums_tail"], new["routes"]
    assert not any("eqa_absmax_slots" in r for r in new["routes"])
    for name in ("activations", "index", "argmax_index", "rotation", "canonicalized", "inverted"):
        assert old[name].dtype == new[name].dtype and old[name].shape == new[name].shape, name
        assert torch.equal(old[name], new[name]), name
    assert new["index"] is new["argmax_index"] or torch.equal(new["index"], new["argmax_index"])


def test_kernel_timer_names_the_new_launches(dev, can, monkeypatch):
    from equiadapt_amd import ops

    x, f = torch.randn(2, 3, 224, 224, device=dev), torch.randn(2, 3, 224, 224, device=dev)
    with ops.KernelTimer() as kt:
        _step(can, x, f, monkeypatch, True)
    names = set(kt.summary())
    assert {"crop_resize_aa_nhwc", "fft_output_partials", "window_sums_tail"} <= names, names
    assert not names & {"crop_resize_aa", "fft_output_sums", "sums_gemv"}, names
    with ops.KernelTimer() as kt:
        _step(can, x, f, monkeypatch, False)
    names = set(kt.summary())
    assert {"crop_resize_aa", "fft_output_sums", "sums_gemv"} <= names, names


def test_a_pixel_written_between_crop_and_network_makes_the_slots_stale(dev, can, monkeypatch):
    """The bound must cover what the lifting kernel reads: after an in-place write the resize kernel's slots no longer do (here the
    new pixel is 50 times the largest), the max pass runs as before, and the activations are those of the old launches on the same crop."""
    from equiadapt_amd import ops
    from equiadapt_amd.images.canonicalization_networks import fftconv

    monkeypatch.setattr(fftconv, "MIN_TILES", 1)
    net = can.canonicalization_network
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(dev)
    acts = {}
    with torch.no_grad():
        for fused in (False, True):
            monkeypatch.setenv("EQA_HEAD_FUSED", "1" if fused else "0")
            monkeypatch.setenv("EQA_TAIL_FUSED", "1" if fused else "0")
            xc = can.transformations_before_canonicalization_network_forward(x)
            assert (ops.crop_absmax_slots(xc) is not None) == fused
            xc[1, 2, 40, 50] = 50.0 * float(xc.abs().max())
            assert ops.crop_absmax_slots(xc) is None
            acts[fused] = net(xc)
            assert "bound:eqa_absmax_slots" in net.last_routes, net.last_routes
            assert net.last_element is None                      # nobody offered tables: the network alone returns activations
    assert torch.isfinite(acts[True]).all()
    assert torch.equal(acts[False], acts[True])
