"""Operands derived from parameters (folded banks, packed weights, filter spectra, packed VNSmall parameters) must follow every kind
of change to their sources -- an in-place write, a storage swap under the same tensor, a replaced tensor object (common/derived.py).

Per network and per kind of change: run the eval fast path once (fills the caches), change one source, run it again, and hold the
second output to the same module's plain route under the rule and tolerance of that network's own parity test.  The output must also
have moved from the first one by more than that tolerance: a change that changes nothing would pass anything.

Shapes: the smallest at which the existing route tests see the fast path taken, at B = 2 -- except ESCNNSteerableNetwork, whose
hidden convolution is on the FFT route (the only one with derived filter spectra) from 8 tiles up: B = 8 at 33 x 33
(test_gpu_fourier_act.py).  Where a network's convolutions have no bias (ESCNNSteerableNetwork, VNSmall) the in-place write goes to
the bias of the first norm instead."""
import copy
import types

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _randomise_norms(net):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)


def _grad_mode_forward(net, x):
    """eval mode with autograd on: every network here leaves its inference fast path and its caches."""
    with torch.enable_grad():
        return net(x).detach().double()


# Each case: (net on the device in eval mode, input, the three tensors' homes, the kernels that show the fast path ran, and
# plain(net, x, monkeypatch) -> (want fp64, elementwise tolerance) evaluated AFTER the change).

def _escnn(dev):
    """test_gpu_parity.py::test_escnn_four_layers_two_winograd_layers' network (lifting MFMA kernel, two Winograd layers, window-sum
    tail); tolerance of test_escnn_inference_fft_path_equals_winograd_and_module_paths against the module path."""
    import equiadapt_amd as ea

    torch.manual_seed(111)
    net = ea.ESCNNEquivariantNetwork((3, 36, 36), 8, 5, "rotation", 8, 4)
    _randomise_norms(net)
    net = net.to(dev).eval()

    def plain(net, x, monkeypatch):
        monkeypatch.setenv("EQA_TRAIN_FAST", "0")                 # autograd on, fused training kernels off: the module sequence
        want = _grad_mode_forward(net, x)
        monkeypatch.delenv("EQA_TRAIN_FAST")
        return want, 2e-5 * max(want.abs().max().item(), 1.0)

    conv, bn = net.eqv_network[0], net.eqv_network[1]
    return types.SimpleNamespace(net=net, x=torch.randn(2, 3, 36, 36, device=dev), bias=conv.bias, bn=bn, param=conv.weights,
                                 kernels=("lift_conv", "winograd_gemm"), plain=plain)


def _wrn(dev):
    """test_gpu_wrn_network.py's network (out_channels = 32, k = 3, 6 layers, C4, 33 x 33) and its rule: the fused route is at most
    4 x as far from the plain route in fp64 as the plain fp32 route is.  The change goes to the first bottleneck's first 1 x 1 layer."""
    import equiadapt_amd as ea

    torch.manual_seed(11)
    net = ea.ESCNNWRNEquivariantNetwork((3, 33, 33), 32, 3, "rotation", 6, 4)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "expanded_weights"):
                m.bias.normal_(0, 0.1)
    _randomise_norms(net)
    net = net.to(dev).eval()

    def plain(net, x, monkeypatch):
        monkeypatch.setenv("EQA_WRN_KERNEL", "0")                 # with autograd on as well: the layers expand their banks anew
        want = _grad_mode_forward(copy.deepcopy(net).double(), x.double())
        d_plain = (_grad_mode_forward(net, x) - want).abs().max().item()
        monkeypatch.delenv("EQA_WRN_KERNEL")
        assert set(net.last_routes) == {"conv2d"}
        return want, 4 * d_plain

    conv, bn = net.eqv_network[3].conv_network[0], net.eqv_network[3].conv_network[1]
    return types.SimpleNamespace(net=net, x=torch.randn(2, 3, 33, 33, device=dev), bias=conv.bias, bn=bn, param=conv.weights,
                                 kernels=("gconv1x1",), plain=plain)


def _convnet(mfma):
    def build(dev):
        """test_gpu_edge_cases.py::test_conv_network_fast_path_in_batch_chunks' network and tolerance, fast path against the module
        sequence: on eqa_conv_s2 (the cached plan), and with EQA_CONVNET_MFMA=0 on the folded convolutions (the cached head)."""
        import equiadapt_amd as ea

        torch.manual_seed(3)
        net = ea.ConvNetwork((3, 64, 64), out_channels=16, kernel_size=5, num_layers=3, out_vector_size=32)
        _randomise_norms(net)
        net = net.to(dev).eval()

        def plain(net, x, monkeypatch):
            want = _grad_mode_forward(net, x)
            return want, 2e-5 * max(want.abs().max().item(), 1.0) + 1e-5 * want.abs()

        conv, bn = net.enc_network[0], net.enc_network[1]
        return types.SimpleNamespace(net=net, x=torch.randn(2, 3, 64, 64, device=dev), bias=conv.bias, bn=bn, param=conv.weight,
                                     kernels=("conv_s2",) if mfma else (), plain=plain, env={} if mfma else {"EQA_CONVNET_MFMA": "0"})
    return build


def _steerable(dev):
    """test_gpu_fourier_act.py::test_network_hidden_layer_on_the_fft_convolution_route's network and rule: the device is at most 4 x
    as far from the fp64 CPU plain-op path as the fp32 CPU plain-op path is (relative to max |out|).  The weights changed are the
    hidden -> hidden convolution's: its cached bank and the spectra derived from it."""
    import equiadapt_amd as ea

    torch.manual_seed(3)
    net = ea.ESCNNSteerableNetwork((3, 33, 33), 16, 7, "rotation", 2)
    x = torch.randn(8, 3, 33, 33)
    with torch.no_grad():
        net.train()
        net(x)
    net = net.to(dev).eval()

    def plain(net, x, monkeypatch):
        host = copy.deepcopy(net).cpu()
        with torch.no_grad():
            want = copy.deepcopy(host).double()(x.cpu().double())
            rel32 = (host(x.cpu()).double() - want).abs().max().item() / want.abs().max().item()
        return want.to(x.device), 4.0 * rel32 * want.abs().max().item()

    return types.SimpleNamespace(net=net, x=x.to(dev), bias=net.block[1].bias, bn=net.block[1], param=net.block[3].weights,
                                 kernels=("fft_gemm", "fourier_elu"), plain=plain)


def _vnsmall(dev):
    """test_gpu_parity.py::test_fused_vnsmall_matches_reference_golden_and_op_path's (2, 300) cloud and tolerance: the fused kernel
    on the packed parameters against the op-by-op module path."""
    import equiadapt_amd as ea

    torch.manual_seed(13)
    net = ea.VNSmall(types.SimpleNamespace(n_knn=20, pooling="mean"))
    _randomise_norms(net)
    net = net.to(dev).eval()

    def plain(net, x, monkeypatch):
        monkeypatch.setenv("EQA_TRAIN_FAST", "0")
        want = _grad_mode_forward(net, x)
        monkeypatch.delenv("EQA_TRAIN_FAST")
        return want, 3e-6 + 1e-4 * want.abs()

    return types.SimpleNamespace(net=net, x=torch.randn(2, 3, 300, device=dev), bias=net.conv_pos.batchnorm.bn2d.bias,
                                 bn=net.conv1.batchnorm.bn1d, param=net.conv1.map_to_feat.weight, kernels=("vnsmall_fwd",), plain=plain)


NETWORKS = {"ESCNNEquivariantNetwork": _escnn, "ESCNNWRNEquivariantNetwork": _wrn, "ConvNetwork": _convnet(True),
            "ConvNetwork-folded": _convnet(False), "ESCNNSteerableNetwork": _steerable, "VNSmall": _vnsmall}


def _bias_written_in_place(case):
    case.bias.add_(0.5)


def _running_mean_replaced(case):
    case.bn.running_mean = case.bn.running_mean.clone() + 0.5


def _parameter_storage_swapped(case):
    version = case.param._version
    case.param.data = case.param.data.clone() * 1.5
    assert case.param._version == version


CHANGES = {"bias_in_place": _bias_written_in_place, "running_mean_replaced": _running_mean_replaced,
           "parameter_storage_swapped": _parameter_storage_swapped}


@pytest.mark.parametrize("change", list(CHANGES))
@pytest.mark.parametrize("network", list(NETWORKS))
def test_fast_path_follows_a_changed_source(dev, network, change, monkeypatch):
    from equiadapt_amd import ops

    case = NETWORKS[network](dev)
    for name, value in getattr(case, "env", {}).items():
        monkeypatch.setenv(name, value)
    with torch.no_grad():
        case.net(case.x)
        before = case.net(case.x).double()                                         # (second call: from the caches)
        CHANGES[change](case)
        with ops.KernelTimer() as timer:
            after = case.net(case.x).double()
        ran = timer.summary()
    assert all(k in ran for k in case.kernels), (case.kernels, sorted(ran))
    want, tol = case.plain(case.net, case.x, monkeypatch)
    err, moved = (after - want).abs(), (after - before).abs()
    print(f"{network} / {change}: max |fast - plain| {err.max().item():.3e}, tolerance {torch.as_tensor(tol).max().item():.3e}, "
          f"moved by {moved.max().item():.3e}")
    assert bool((moved > tol).any()), "the change did not move the output: the case shows nothing"
    assert bool((err <= tol).all()), (err.max().item(), torch.as_tensor(tol).max().item())
