"""common/derived.py: the one rule for "a source tensor is unchanged" (same object, same ``_version``, same ``data_ptr()``), the cache
built on it, and the eval-mode batch-norm affine that six sites share."""
import pytest
import torch

from equiadapt_amd.common.derived import DerivedCache, bn_eval_affine


class Counted:
    """build(): a fresh object per call, counting the calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def test_an_unchanged_stamp_returns_the_same_object_without_building_again():
    cache, build = DerivedCache(), Counted()
    w, b = torch.randn(4, 3), torch.randn(4)
    first = cache.get("slot", (w, b, None), build, (3, 8, 8), "f32")
    assert "slot" in cache and "other" not in cache
    for _ in range(3):
        assert cache.get("slot", (w, b, None), build, (3, 8, 8), "f32") is first
    assert cache.get("slot", [w, b, None], build, (3, 8, 8), "f32") is first          # a list of the same objects is the same sources
    assert build.calls == 1
    cache.clear()
    assert "slot" not in cache and cache.get("slot", (w, b, None), build, (3, 8, 8), "f32") is not first and build.calls == 2


def _in_place(src):
    src["w"].add_(1.0)


def _storage_swap(src):
    version = src["w"]._version
    src["w"].data = src["w"].data.clone()
    assert src["w"]._version == version                       # what a key on _version alone cannot see


def _replaced_object(src):
    old = src["w"]
    src["w"] = old.clone()
    assert src["w"]._version == old._version and torch.equal(src["w"], old)       # equal value, equal version, another object


def _none_becomes_a_tensor(src):
    src["b"] = torch.zeros(4)


def _tensor_becomes_none(src):
    assert src["b"] is not None                               # (a tensor in this case: see the parametrisation)
    src["b"] = None


@pytest.mark.parametrize("change,bias", [(_in_place, None), (_storage_swap, None), (_replaced_object, None),
                                         (_none_becomes_a_tensor, None), (_tensor_becomes_none, torch.ones(4))])
def test_every_kind_of_change_to_a_source_forces_a_rebuild(change, bias):
    cache, build = DerivedCache(), Counted()
    src = {"w": torch.randn(4, 3), "b": bias}
    first = cache.get("slot", (src["w"], src["b"]), build)
    assert cache.get("slot", (src["w"], src["b"]), build) is first and build.calls == 1
    change(src)
    second = cache.get("slot", (src["w"], src["b"]), build)
    assert second is not first and build.calls == 2
    assert cache.get("slot", (src["w"], src["b"]), build) is second and build.calls == 2


def test_a_none_source_becoming_a_tensor_and_back_rebuilds_both_times():
    cache, build = DerivedCache(), Counted()
    w, b = torch.randn(4, 3), torch.zeros(4)
    for n, bias in enumerate((None, b, None), start=1):
        value = cache.get("slot", (w, bias), build)
        assert build.calls == n and cache.get("slot", (w, bias), build) is value and build.calls == n


def test_a_changed_context_value_forces_a_rebuild():
    cache, build = DerivedCache(), Counted()
    w = torch.randn(4, 3)
    first = cache.get("plan", (w,), build, (3, 64, 64), 4)
    assert cache.get("plan", (w,), build, (3, 64, 64), 4) is first
    assert cache.get("plan", (w,), build, (3, 32, 32), 4) is not first and build.calls == 2
    assert cache.get("plan", (w,), build, (3, 32, 32), 2) is not first and build.calls == 3
    assert cache.get("plan", (w,), build, (3, 32, 32)) is not first and build.calls == 4


def test_derived_is_rebuilt_when_and_only_when_its_parent_entry_was():
    cache, fold, spectra, other = DerivedCache(), Counted(), Counted(), Counted()
    w, v = torch.randn(4, 3), torch.randn(2)

    def step():
        return cache.get("conv", (w,), fold), cache.derived("conv", ("conv", "fft"), spectra), cache.get("other", (v,), other)

    bank, fft, _ = step()
    assert step()[:2] == (bank, fft) and (fold.calls, spectra.calls, other.calls) == (1, 1, 1)
    v.add_(1.0)                                               # another slot of the same cache is rebuilt: the derived entry is kept
    assert step()[:2] == (bank, fft) and (fold.calls, spectra.calls, other.calls) == (1, 1, 2)
    w.add_(1.0)                                               # the parent is rebuilt: so is what was made from it
    bank2, fft2, _ = step()
    assert bank2 is not bank and fft2 is not fft and (fold.calls, spectra.calls, other.calls) == (2, 2, 2)
    assert step()[:2] == (bank2, fft2) and (fold.calls, spectra.calls) == (2, 2)
    w.data = w.data.clone()                                   # a parent rebuilt to an EQUAL stamp tuple would still be another entry
    assert step()[1] is not fft2 and (fold.calls, spectra.calls) == (3, 3)


def test_derived_of_a_missing_parent_is_an_error():
    with pytest.raises(KeyError):
        DerivedCache().derived("conv", ("conv", "fft"), Counted())


def test_a_deep_copy_of_a_module_does_not_serve_the_original_operands():
    """The tests and users copy.deepcopy networks whose caches are filled: the copy's entries must follow the copy's own tensors."""
    import copy

    import equiadapt_amd as ea

    torch.manual_seed(0)
    net = ea.ConvNetwork((3, 16, 16), 4, 3, 2, 8).eval()
    conv, bn = net.enc_network[0], net.enc_network[1]
    with torch.no_grad():
        w, b = net._folded(conv, bn)
        assert net._folded(conv, bn)[0] is w
        twin = copy.deepcopy(net)
        twin.enc_network[0].weight.mul_(2.0)
        w2, b2 = twin._folded(twin.enc_network[0], twin.enc_network[1])
        assert torch.equal(w2, 2.0 * w) and torch.equal(b2, b) and net._folded(conv, bn)[0] is w


def test_bn_eval_affine_is_the_written_out_expression_bit_for_bit():
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm2d(37).eval()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.3)
        bn.bias.normal_(0.0, 0.3)
        bn.running_mean.normal_(0.0, 0.5)
        bn.running_var.uniform_(0.2, 3.0)
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    shift = bn.bias - bn.running_mean * scale
    got_scale, got_shift = bn_eval_affine(bn)
    assert torch.equal(got_scale, scale) and torch.equal(got_shift, shift)
    x = torch.randn(5, 37, 3, 3)
    # and it is the module's eval forward, to fp32 rounding of values up to ~25 (four roundings of 2^-24 each)
    assert torch.allclose(bn(x), x * scale[None, :, None, None] + shift[None, :, None, None], rtol=0, atol=4 * 25 * 2.0 ** -24)
