"""CPU-only: the C-ABI library loads and exports every symbol of include/eqa_hip.h; host-side tables."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    text = open(os.path.join(ROOT, "include", "eqa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eqa_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from equiadapt_amd import _lib

    _lib.build()
    names = _header_functions()
    assert len(names) >= 10
    assert sorted(_lib.SIGNATURES) == names, "ctypes SIGNATURES and include/eqa_hip.h disagree"
    lib = ctypes.CDLL(_lib.SO_PATH)
    for n in names:
        assert hasattr(lib, n), f"libeqa_hip.so does not export {n}"
    # the version the library reports == the header's macro == the binding's constant (bumped whenever entry points are added)
    macro = int(re.search(r"#define\s+EQA_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "eqa_hip.h")).read()).group(1))
    assert _lib.load().eqa_abi_version() == macro == _lib.ABI_VERSION == 3
    # host-side constants that mirror compiled ones are read back from the library (no compute: a getter)
    from equiadapt_amd import ops

    assert _lib.load().eqa_get_option(100) == ops.MAX_WINDOW_K
    header = open(os.path.join(ROOT, "include", "eqa_hip.h")).read()
    assert ops.VNSMALL_PARAMS == int(re.search(r"#define\s+EQA_VNSMALL_PARAMS\s+(\d+)", header).group(1))
    assert ops.VNSMALL_PARAMS_MAX == int(re.search(r"#define\s+EQA_VNSMALL_PARAMS_MAX\s+(\d+)", header).group(1))
    # argument validation happens before any device work, so it is checkable without a GPU
    assert _lib.load().eqa_set_option(99, 0) == -1
    assert _lib.load().eqa_group_pool_workspace_bytes(4, 32, 8, 7056) > 0


def test_ops_refuse_cpu_tensors_loudly():
    from equiadapt_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.so3_rotate(torch.zeros(1, 3, 4), torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.group_argmax(torch.zeros(2, 4))


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    from equiadapt_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.EqaLibraryError, match="no CPU fallback"):
        _lib.load()


def test_theta_tables_equal_the_oracle_chain():
    """The product's tables are bit-identical to what the oracle's kornia restatement gives affine_grid."""
    from equiadapt_amd.images import geometry as g
    from oracle import image_ops as io

    for N, hw in [(8, (448, 448)), (4, (64, 48)), (8, (224, 224)), (6, (30, 31))]:
        ang = g.group_angles(N)
        assert torch.equal(ang, io.group_angles(N))
        for sign in (1.0, -1.0):
            c = torch.tensor([float(hw[1] - 1) / 2, float(hw[0] - 1) / 2]).expand(N, -1)
            ref = io.kornia_affine_theta(io.kornia_rotation_matrix2d(c, sign * ang), hw, hw).reshape(N, 6)
            assert torch.equal(g.rotation_theta(sign * ang, hw), ref)


def test_invert_channel_map_is_roll_by_gather():
    from equiadapt_amd.images import geometry as g
    from oracle import image_ops as io

    for N, refl in [(4, False), (8, False), (4, True), (6, True), (6, False)]:
        E = 2 * N if refl else N
        theta, flags, cmap = g.invert_tables(N, refl, (8, 8))
        assert theta.shape == (E, 6) and cmap.shape == (E, E)
        x = torch.arange(E, dtype=torch.float32).view(1, 1, E, 1, 1)
        for e in range(E):
            ang = g.group_angles(N)[e % N].reshape(1)
            shift = ang / 360.0 * N
            if refl:
                want = torch.cat([io.roll_by_gather(x[:, :, :N], shift), io.roll_by_gather(x[:, :, N:], -shift)], dim=2)
                assert flags[e].item() == (g.FLIP_DST if e < N else 0)  # flipped when the indicator is 0
            else:
                want = io.roll_by_gather(x, shift)
            assert want.flatten().long().tolist() == cmap[e].tolist(), (N, refl, e)


def test_canonicalize_and_orbit_flags():
    from equiadapt_amd.images import geometry as g

    th, fl = g.canonicalize_tables(4, True, (16, 16))
    assert fl.tolist() == [0] * 4 + [g.FLIP_SRC] * 4 and torch.equal(th[:4], th[4:])
    th, fl = g.orbit_tables(4, True, (16, 16))
    assert fl.tolist() == [0] * 4 + [g.FLIP_DST] * 4
    assert g.center_crop_offset(225, 180) == 22 and g.center_crop_offset(227, 180) == 24  # round-half-even


def test_reference_shape_contract_pre_transform():
    """reference tests/images/canonicalization/test_continuous_group.py:89-91: (1,3,64,64) -> (1,3,32,32)."""
    from equiadapt_amd.images.transforms import CenterCrop, Resize

    x = torch.randn(1, 3, 64, 64)
    assert Resize(32)(CenterCrop(58)(x)).shape == (1, 3, 32, 32)


def test_aa_resize_tables_reproduce_torch_interpolate():
    """Host tables of eqa_crop_resize_aa applied with plain torch on the CPU == CenterCrop + F.interpolate(antialias)."""
    import math

    from equiadapt_amd.images import geometry as g
    from oracle import image_ops as io

    torch.manual_seed(0)
    for (H, W, ratio, size) in [(224, 224, 0.8, 96), (64, 64, 0.9, 32), (50, 70, 0.8, (24, 40)), (33, 33, 1.0, 17),
                                (64, 64, 0.9, 64), (40, 52, 0.7, (61, 80))]:   # up-sampling: the tutorial's 58 -> 64, and both axes by 2.2
        x = torch.randn(2, 3, H, W)
        crop = (math.ceil(H * ratio), math.ceil(W * ratio))
        out_hw = io.tv_resize_output_size(crop, size)
        wx, x0, wy, y0, K, max_rows = g.aa_resize_tables((H, W), crop, out_hw)[:6]
        cols = (x0[:, None].long() + torch.arange(K)[None, :]).clamp(max=W - 1)      # (OW, K)
        tmp = (x[:, :, :, cols] * wx[None, None, None]).sum(-1)                      # horizontal pass (B,C,H,OW)
        rows = (y0[:, None].long() + torch.arange(K)[None, :]).clamp(max=H - 1)      # (OH, K)
        got = (tmp[:, :, rows, :] * wy[None, None, :, :, None]).sum(3)               # vertical pass (B,C,OH,OW)
        want = io.pre_canonicalization_transform(x, (3, H, W), ratio, size)
        assert got.shape == want.shape and (got - want).abs().max().item() < 2e-6
        assert max_rows >= 1


def test_mask_rotation_table_matches_torchvision_restatement():
    from equiadapt_amd.images import geometry as g

    t = g.mask_rotation_table([0.0, 90.0], (8, 12))
    assert t.shape == (2, 6)
    assert torch.allclose(t[0], torch.tensor([1 / 6.0, 0.0, 0.0, 0.0, 1 / 4.0, 0.0]), atol=1e-7)


def test_winograd_cook_toom_matrices_are_exact():
    """F(2,5) and F(4,5): y = A^T[(G g) * (B^T d)] equals the 5-tap correlation in rational arithmetic, B^T and A^T are
    dyadic (exact in fp32), and g_matrix carries the sign convention of the kernels' B^T rows."""
    import random
    from fractions import Fraction

    from equiadapt_amd.images.canonicalization_networks import winograd as w

    rng = random.Random(5)
    for m in (2, 4):
        at, g, bt = w.cook_toom(m)
        n = m + 4
        assert len(bt) == n and len(g) == n and len(at) == m
        for _ in range(5):
            d = [Fraction(rng.randint(-99, 99)) for _ in range(n)]
            f = [Fraction(rng.randint(-99, 99)) for _ in range(5)]
            U = [sum(g[k][j] * f[j] for j in range(5)) for k in range(n)]
            V = [sum(bt[k][j] * d[j] for j in range(n)) for k in range(n)]
            y = [sum(at[i][k] * U[k] * V[k] for k in range(n)) for i in range(m)]
            assert y == [sum(d[i + j] * f[j] for j in range(5)) for i in range(m)]
        for row in bt + at:
            for v in row:
                assert v.denominator in (1, 2, 4, 8), v   # dyadic: the on-the-fly transforms add no representation error
        G = w.g_matrix(m)
        sg = w.kernel_bt_signs(m)
        assert G.shape == (n, 5) and G.dtype == torch.float64
        for k in range(n):
            assert [float(sg[k] * v) for v in g[k]] == G[k].tolist()
        U = w.transform_filters(torch.randn(3, 2, 5, 5), m)
        assert U.shape == (n * n, 2, 3) and U.dtype == torch.float32


def test_continuous_group_host_geometry():
    """warp_affine_theta == kornia's normalise / invert chain (oracle restatement); the half-pixel conversion reproduces
    F.affine_grid(align_corners=False) sampling positions under align_corners=True arithmetic."""
    import torch.nn.functional as F

    from equiadapt_amd.images import geometry
    from oracle import image_ops as o

    torch.manual_seed(3)
    for (Hp, Wp) in [(40, 48), (33, 33), (448, 448)]:
        R = o.steerable_rotation_from_vector(torch.randn(6, 2))
        R[:, [0, 1], [1, 0]] *= -1
        alpha, beta = R[:, 0, 0], R[:, 0, 1]
        cx, cy = Hp // 2, Wp // 2
        M = torch.cat([R, torch.stack([(1 - alpha) * cx - beta * cy, beta * cx + (1 - alpha) * cy], 1).unsqueeze(-1)], -1)
        got = geometry.warp_affine_theta(M, (Hp, Wp))
        want = o.kornia_affine_theta(M, (Hp, Wp), (Hp, Wp)).reshape(6, 6)
        assert torch.allclose(got, want, atol=2e-6)
        th = torch.randn(4, 2, 3) * 0.5
        g = F.affine_grid(th, [4, 1, Hp, Wp], align_corners=False)
        g2 = F.affine_grid(geometry.affine_grid_theta_half_pixel(th, (Hp, Wp)).reshape(4, 2, 3), [4, 1, Hp, Wp], align_corners=True)
        ix_f, iy_f = ((g[..., 0] + 1) * Wp - 1) / 2, ((g[..., 1] + 1) * Hp - 1) / 2
        ix_t, iy_t = (g2[..., 0] + 1) * (Wp - 1) / 2, (g2[..., 1] + 1) * (Hp - 1) / 2
        assert (ix_f - ix_t).abs().max() < 1e-4 * Wp / 40 and (iy_f - iy_t).abs().max() < 1e-4 * Hp / 40
    # differentiable
    M = M.clone().requires_grad_(True)
    geometry.warp_affine_theta(M, (Hp, Wp)).sum().backward()
    assert torch.isfinite(M.grad).all()


def test_continuous_group_reference_api_cases():
    """The reference's own tests for this class (tests/images/canonicalization/test_continuous_group.py:52-91): construction
    and the (1,3,64,64) -> (1,3,32,32) pre-transform, hyper-parameters given as a mapping or by attribute."""
    import types

    import equiadapt_amd as ea

    for hp in ({"input_crop_ratio": 0.9, "resize_shape": (32, 32)},
               types.SimpleNamespace(input_crop_ratio=0.9, resize_shape=(32, 32))):
        c = ea.ContinuousGroupImageCanonicalization(torch.nn.Identity(), hp, (3, 64, 64))
        assert c.pad is not None and c.crop is not None
        out = c.transformations_before_canonicalization_network_forward(torch.rand(1, 3, 64, 64))
        assert out.size() == torch.Size([1, 3, 32, 32])
        with pytest.raises(NotImplementedError):
            c.get_groupelement(torch.rand(1, 3, 64, 64))
    g = ea.ContinuousGroupImageCanonicalization(torch.nn.Identity(), hp, (1, 28, 28))
    assert isinstance(g.pad, torch.nn.Identity) and isinstance(g.resize_canonization, torch.nn.Identity) and g.pad_size == 0


def test_update_running_stats_matches_nn_batchnorm():
    """common.utils.update_running_stats == what nn.BatchNorm2d does to its buffers in a training forward, for a numeric
    momentum, for momentum=None (cumulative average) and with track_running_stats=False."""
    from equiadapt_amd.common.utils import update_running_stats

    torch.manual_seed(4)
    for momentum in (0.1, 0.9, None):
        a, b = torch.nn.BatchNorm2d(5, momentum=momentum), torch.nn.BatchNorm2d(5, momentum=momentum)
        for _ in range(3):
            x = torch.randn(4, 5, 6, 7) * 2 + 1
            a.train()(x)
            update_running_stats(b, x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=True))
        assert torch.allclose(a.running_mean, b.running_mean, atol=1e-6) and torch.allclose(a.running_var, b.running_var, atol=1e-5)
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 3
    c = torch.nn.BatchNorm2d(5, track_running_stats=False)
    update_running_stats(c, torch.zeros(5), torch.ones(5))          # no buffers: nothing to do, must not raise
    assert c.running_mean is None


def test_fft_filter_spectra_real_form_reproduces_conv2d():
    """Host side of the FFT convolution (fftconv.filter_spectra): with the tile spectra taken by torch.fft in the layout the
    kernels write -- V[f][m] = [Re | Im] over channels, f = ky*25 + kx -- the real-form batched product and the inverse
    transform give conv2d.  Pins the [[Br, Bi], [-Bi, Br]] block layout, the conjugate (cross-correlation) and the 1/48^2."""
    import torch.nn.functional as F

    from equiadapt_amd.images.canonicalization_networks import fftconv

    torch.manual_seed(3)
    B, Cin, Cout = 2, 3, 5
    x = torch.randn(B, Cin, 48, 48, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 5, 5, dtype=torch.float64)
    Bm = fftconv.filter_spectra(w.float(), groups=(Cin, Cout)).double()     # (F, 2 Cin, 2 Cout), plain [Re | Im] order
    X = torch.fft.rfft2(x)                                                  # (B, Cin, 48, 25)
    ky, kx = fftconv.freq_index()                                           # the F = 1154 stored frequencies, kernels' order
    assert len(ky) == fftconv.F == 1154
    Xs = X[:, :, ky, kx]                                                    # (B, Cin, F)
    V = torch.cat([Xs.real, Xs.imag], dim=1).permute(2, 0, 1).contiguous()  # (F, B, 2 Cin)
    Mo = torch.bmm(V, Bm)                                                   # (F, B, 2 Cout)
    Ys = torch.complex(Mo[..., :Cout], Mo[..., Cout:]).permute(1, 2, 0)     # (B, Cout, F)
    Y = torch.zeros(B, Cout, 48, 25, dtype=torch.complex128)
    Y[:, :, ky, kx] = Ys
    for col in (0, 24):                                                     # the dropped halves of the two edge columns
        Y[:, :, 25:, col] = Y[:, :, 1:24, col].flip(2).conj()
    y = torch.fft.irfft2(Y, s=(48, 48)) * (48 * 48)                         # the spectra carry 1/48^2; irfft2 divides again
    want = F.conv2d(x, w)
    assert (y[:, :, :44, :44] - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    assert fftconv.tiles(92) == 2 and fftconv.tiles(48) == 1 and fftconv.tiles(49) == 2 and fftconv.tiles(4) == 0
    # interleaved orders: groups of G channels, [Re x G | Im x G] each -- a permutation of the plain order
    o = fftconv._order(32, 8)
    assert sorted(o.tolist()) == list(range(64)) and o[:16].tolist() == list(range(8)) + list(range(32, 40))
    assert fftconv._order(3, 1).tolist() == [0, 3, 1, 4, 2, 5]                      # re/im interleaved: the kernels' layout
    wq = torch.randn(4, 3, 5, 5)
    Bi, Bp = fftconv.filter_spectra(wq, groups=(1, 1)), fftconv.filter_spectra(wq, groups=(3, 4))
    assert Bi.shape == (fftconv.F, 6, 8) and torch.equal(Bi, Bp[:, fftconv._order(3, 1)][:, :, fftconv._order(4, 1)])
    assert fftconv.group_sizes(256, 256) == (16, 1) and fftconv.group_sizes(12, 8) == (1, 1)


def test_fft_group_rule_matches_the_library():
    """The [Re | Im] grouping of V's rows is decided in two places (fftconv.group_sizes for the filter spectra, the library for
    the kernels): they must agree."""
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    for c in (4, 12, 16, 64, 250, 256):
        assert (lib.eqa_fft48k5_group(c, 0), lib.eqa_fft48k5_group(c, 1)) == fftconv.group_sizes(c, c)
    assert lib.eqa_fft48k5_frequencies() == fftconv.F


def test_generated_fft48_is_current_and_correct():
    """csrc/fft48.inc is generated (tools/gen_fft48.py): the committed file equals what the generator renders now, and the
    operation list, run in numpy with fp32 rounding, is the 48-point DFT (vs numpy.fft, forward and -- with re / im swapped --
    inverse)."""
    import importlib.util
    import os

    import numpy as np

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_fft48", os.path.join(root, "tools", "gen_fft48.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render() == open(os.path.join(root, "equiadapt_amd", "csrc", "fft48.inc")).read()
    rng = np.random.default_rng(1)
    for _ in range(3):
        z = rng.standard_normal(48) + 1j * rng.standard_normal(48)
        want = np.fft.fft(z)
        assert np.abs(gen.evaluate(z) - want).max() <= 4e-6 * np.abs(want).max()
        sw = gen.evaluate(z.imag + 1j * z.real)                      # inverse = forward on swapped parts, swapped back
        inv = sw.imag + 1j * sw.real
        assert np.abs(inv - np.fft.ifft(z) * 48).max() <= 4e-6 * np.abs(want).max()


def test_escnn_network_refuses_e2cnn_checkpoints_with_a_pointer_to_the_bridge():
    """A reference checkpoint (e2cnn steerable-basis parameters) must fail with an explanation, not with a shape mismatch."""
    import pytest
    import torch

    import equiadapt_amd as ea

    net = ea.ESCNNEquivariantNetwork((3, 32, 32), 2, 3, "rotation", 4, 2)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)                                     # its own state dict loads
    bad = dict(sd)
    bad["eqv_network.0.weights"] = torch.zeros(24)              # e2cnn: one flat coefficient vector per layer
    bad["eqv_network.0.basisexpansion.block_expansion_('irrep_0', 'regular').sampled_basis"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="load_exported_dense"):
        net.load_state_dict(bad, strict=False)


def test_public_surface_holds_every_on_path_name_of_the_reference():
    """`import equiadapt_amd as equiadapt` must resolve every name of the reference's top-level ``__all__``
    (equiadapt/__init__.py:52-96, listed here as data) that SURVEY.md section 8 puts on the hot path; the names left out are
    listed with the reason, so a new omission fails the test."""
    import types as _types

    import equiadapt_amd as ea

    reference_all = [
        "BaseCanonicalization", "ContinuousGroupCanonicalization", "ContinuousGroupImageCanonicalization",
        "ContinuousGroupPointcloudCanonicalization", "ConvNetwork", "CustomEquivariantNetwork", "DiscreteGroupCanonicalization",
        "DiscreteGroupImageCanonicalization", "ESCNNEquivariantNetwork", "ESCNNSteerableNetwork", "ESCNNWRNEquivariantNetwork",
        "ESCNNWideBasic", "ESCNNWideBottleneck", "EquivariantPointcloudCanonicalization", "GroupEquivariantImageCanonicalization",
        "IdentityCanonicalization", "LieParameterization", "OptimizedGroupEquivariantImageCanonicalization",
        "OptimizedSteerableImageCanonicalization", "ResNet18Network", "RotationEquivariantConv", "RotationEquivariantConvLift",
        "RotoReflectionEquivariantConv", "RotoReflectionEquivariantConvLift", "SteerableImageCanonicalization", "VNBatchNorm",
        "VNBilinear", "VNLeakyReLU", "VNLinear", "VNLinearLeakyReLU", "VNMaxPool", "VNSmall", "VNSoftplus", "VNStdFeature",
        "basecanonicalization", "custom_equivariant_networks", "custom_group_equivariant_layers", "custom_nonequivariant_networks",
        "equivariant_networks", "escnn_networks", "get_action_on_image_features", "get_graph_feature_cross", "gram_schmidt",
    ]
    off_path = {
        # e2cnn internals that cannot be restated here (SURVEY section 2 "(f)", DESIGN section 1 "out of scope")
        "ESCNNSteerableNetwork", "ESCNNWRNEquivariantNetwork", "ESCNNWideBasic", "ESCNNWideBottleneck",
        # torchvision-pretrained prediction-side network, not a canonicalization hot path
        "ResNet18Network",
        # Lie-algebra parameterisation of the continuous groups: no caller on the path
        "LieParameterization",
        # vector-neuron layers VNSmall does not use (vector_neuron_layers.py:15-207, 383-492)
        "VNBilinear", "VNLeakyReLU", "VNLinear", "VNSoftplus", "VNStdFeature",
    }
    on_path = [n for n in reference_all if n not in off_path]
    missing = [n for n in on_path if not hasattr(ea, n)]
    assert not missing, missing
    assert set(on_path) <= set(ea.__all__)
    for n in ("basecanonicalization", "custom_equivariant_networks", "custom_group_equivariant_layers", "custom_nonequivariant_networks",
              "equivariant_networks", "escnn_networks"):
        assert isinstance(getattr(ea, n), _types.ModuleType), n
    assert ea.custom_group_equivariant_layers.RotationEquivariantConvLift is ea.RotationEquivariantConvLift
    assert ea.equivariant_networks.VNSmall is ea.VNSmall


def test_variant_build_needs_its_own_output_path():
    from equiadapt_amd import _lib

    with pytest.raises(ValueError):
        _lib.build(extra_flags=["-DEQA_ABL_NOMASK"])


def test_eight_concurrent_builders_on_a_stale_tree_leave_one_intact_library(tmp_path):
    """The first run of `bench.py --gpus 8` (or of pytest-xdist) on a stale tree: eight processes call _lib.build() at the same time.
    With a stand-in compiler (a script that takes 0.2 s per object and concatenates at link time) on a scratch copy of the build
    inputs: every process returns the library path, the library holds every translation unit exactly once and was linked ONCE (the
    others queue on csrc/_obj/.lock and find it fresh), no compile temporaries and no foreign objects are left -- and an unrelated
    live process's temporary survives the cleanup while a dead one's is removed (the cleanup used to delete both)."""
    import subprocess
    import sys
    import textwrap

    csrc = tmp_path / "csrc"
    (csrc / "_obj").mkdir(parents=True)
    names = [f"unit{i}.hip" for i in range(6)]
    for n in names:
        (csrc / n).write_text(f"// {n}\n")
    (csrc / "common.hpp").write_text("// header\n")
    fake = tmp_path / "fakecc"
    fake.write_text(textwrap.dedent("""\
        #!/usr/bin/env python3
        import sys, time, os
        a = sys.argv[1:]
        out = a[a.index("-o") + 1]
        if "-c" in a:
            time.sleep(0.2)
            src = a[a.index("-c") + 1]
            open(out, "w").write("OBJ " + os.path.basename(src) + "\\n")
        else:
            objs = [x for x in a if x.endswith(".o")]
            time.sleep(0.2)
            with open(os.path.join(os.path.dirname(out), "link_count"), "a") as f:
                f.write("1\\n")
            open(out, "w").write("".join(open(o).read() for o in objs))
        """))
    fake.chmod(0o755)
    live = csrc / "_obj" / f"unit0.deadbeef00.o.tmp{os.getpid()}"              # this (live) process's in-flight temporary
    live.write_text("in flight")
    dead = csrc / "_obj" / "unit0.deadbeef00.o.tmp999999999"                   # no such pid
    dead.write_text("orphan")
    stale = csrc / "_obj" / "unit0.0123456789.o"                                # another flag set's finished object, old
    stale.write_text("old variant")
    os.utime(stale, (1, 1))
    child = textwrap.dedent(f"""\
        import os, sys
        sys.path.insert(0, {ROOT!r})
        from equiadapt_amd import _lib
        _lib.CSRC = {str(csrc)!r}
        _lib.SOURCES = [os.path.join(_lib.CSRC, n) for n in {names!r}]
        _lib.HEADERS = [os.path.join(_lib.CSRC, "common.hpp")]
        _lib.SO_PATH = os.path.join(_lib.CSRC, "libfake.so")
        print(_lib.build())
        """)
    env = dict(os.environ, HIPCC=str(fake))
    procs = [subprocess.Popen([sys.executable, "-c", child], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(8)]
    outs = [p.communicate(timeout=120) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se
        assert so.strip().endswith("libfake.so")
    lib = (csrc / "libfake.so").read_text().splitlines()
    assert sorted(lib) == sorted(f"OBJ {n}" for n in names)
    assert (csrc / "link_count").read_text().count("1") == 1
    left = sorted(os.listdir(csrc / "_obj"))
    assert live.name in left and dead.name not in left and stale.name not in left
    assert [n for n in left if ".o.tmp" in n] == [live.name]
    assert len([n for n in left if n.endswith(".o")]) == len(names)


def test_gemm_form_rule_and_fp16_weight_pieces_on_the_host():
    """Host logic of round 6's fp16 forms, no GPU: which contraction `fftconv.gemm_form` picks, and the operand `LiftedInput.pieces_f16`
    builds for eqa_lift5_fft48k5_input_f16x2 -- layout (C, 2 pieces, 5 filter rows, 4 chunks, 8), zero slots, a power-of-two scale that
    takes max |w| into [2^13, 2^14], and h1 + h2 within one fp32 ulp of the scaled weight."""
    import math

    import torch

    from equiadapt_amd.images.canonicalization_networks import fftconv

    if fftconv.GEMM_PIECES == "auto":
        assert fftconv.gemm_form(256, 256) == "6" and fftconv.gemm_form(256, 256, True) == "h3"
        assert fftconv.gemm_form(64, 128, True) == "h3" and fftconv.gemm_form(64, 128) == "f32"
        assert fftconv.gemm_form(32, 128, True) == "f32" and fftconv.gemm_form(256, 64, True) == "f32" and fftconv.gemm_form(80, 128, True) == "f32"
    torch.manual_seed(0)
    bank = torch.randn(32, 3, 5, 5) * 0.37
    x = torch.zeros(1, 3, 16, 16)
    wh, scale = fftconv.LiftedInput(x, bank, None, True).pieces_f16()
    assert wh.shape == (32, 2, 5, 4, 8) and wh.dtype == torch.float16
    assert math.frexp(scale)[0] == 0.5 and 2.0 ** 13 <= bank.abs().max().item() * scale <= 2.0 ** 14
    assert (wh[:, :, :, 3] == 0).all() and (wh[..., 3] == 0).all() and (wh[..., 7] == 0).all() and (wh[:, :, :, 0, :4] == 0).all()
    # chunk p of filter row ky = [w(:, kx = 2p - 1), 0, w(:, kx = 2p), 0]
    got = (wh[:, 0].double() + wh[:, 1].double()).reshape(32, 5, 8, 4)[:, :, 1:6, :3].permute(0, 3, 1, 2)      # (C, ci, ky, kx)
    want = bank.double() * scale
    # |x - h1 - h2| <= 2^-23 |x| element by element (one fp32 ulp at worst), a third of that in rms; + the fp16 subnormal step
    err = (got - want).abs()
    assert (err <= 2.0 ** -23 * want.abs() + 2.0 ** -24).all()
    nz = want.abs() > 0
    assert (err[nz] / want.abs()[nz]).pow(2).mean().sqrt().item() <= 0.5 * 2.0 ** -23
