"""CPU: the single-channel spectral domains of the resolution discriminators ('linear' / 'log': csrc/spectral.hip mrd_image1_*,
the C_in = 1 first convolution through the direct kernels of csrc/conv.hip and csrc/conv_wgrad.hip) on the kernel interpreter
(cases and bounds: tests/_mrdcases.py, tests/_convcases.py; the same and the model-level checks on the GPU:
tests/test_gpu_mrd_domains.py)."""
import os
import subprocess

import pytest
import torch

import _convcases
import _mrdcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu', 'libmsmc_emu.so')
DEV = 'cpu'

# the first layer of DiscriminatorR with one input channel: 3 x 3, reflection-padded, C_out = hidden / 32 of the shipped widths
# (128 / 256 / 512 -> 4 / 8 / 16) and of the small fixture (32 -> 1); odd sizes, more than one block of 256 points
# (name, B, Cin, Cout, H, W, kernel, stride, dilation, padding, reflect, in_slope)
LAYER0 = [('mrd1 1->%d s1' % co, 2, 1, co, 9, 37, (3, 3), (1, 1), (1, 1), (1, 1), True, 1.0) for co in (1, 4, 8, 16)]


@pytest.fixture(scope='module', autouse=True)
def emulator():
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tests', 'emu')])
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok)
    lib.use_library_for_tests(EMU)
    assert lib.backend() == 'emu'
    yield
    lib._lib, lib._host_pointers_ok = saved


def _waveform():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 610, generator=g)
    x[1] *= torch.exp(-torch.arange(610.0) / 610.0 * 12.0)
    return x


def test_single_channel_image_is_that_channel_of_the_two_channel_image_bit_for_bit():
    _mrdcases.check_image_exact(DEV, _waveform(), (15, 50))


def test_single_channel_image_backward_matches_autograd_across_both_clamp_edges():
    _mrdcases.check_image_backward(DEV)


def test_single_channel_image_unaligned_operands_and_refusals():
    _mrdcases.check_image_unaligned_and_refusals(DEV)


def test_front_ends_in_lock_step_equal_the_chains_one_by_one_for_every_domain():
    _mrdcases.check_lockstep(DEV, _waveform(), (15, 50))


@pytest.mark.parametrize('dtype,tol', [(torch.float32, 2e-4), (torch.bfloat16, 2e-2)], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', LAYER0, ids=[c[0] for c in LAYER0])
def test_first_convolution_with_one_input_channel(case, dtype, tol):
    """forward, data gradient and weight gradient against F.conv2d on the reflection-padded input, at the bounds of the
    interpreter's convolution cases (tests/test_product_emu.py test_conv_kernels_small_and_thin_shapes: 2e-4 fp32, 2e-2 bf16)"""
    _convcases.check_conv_case(case, dtype, tol, DEV)


def test_first_convolution_with_one_input_channel_takes_the_direct_kernels():
    """C_in = 1 is an instantiation of the direct small-channel kernel (CI = 1), not a padded two-channel image"""
    from msmctts_amd.hip import lib
    for case, want in ((LAYER0[1], 'conv_direct_small_kernel<float, 1, 4, 0>'), (LAYER0[2], 'conv_direct_small_kernel<float, 1, 8, 0>')):
        _convcases.check_conv_case(case, torch.float32, 2e-4, DEV, parts=('fwd',))
        assert lib.get().msmc_conv_last_kernel().decode() == want
        _convcases.check_conv_case(case, torch.float32, 2e-4, DEV, parts=('dgrad',))
        assert lib.get().msmc_conv_last_kernel().decode().startswith('conv_direct_small_kernel<float, %d, 1' % case[3])


def test_unknown_domain_is_refused_at_construction():
    from msmctts_amd.networks.hifigan.discriminator import Discriminator, MultiResolutionDiscriminator
    from msmctts_amd.utils.audio import TorchSTFT
    with pytest.raises(ValueError, match='cepstral'):
        TorchSTFT(60, 15, 60, domain='cepstral')
    with pytest.raises(ValueError, match='cepstral'):
        MultiResolutionDiscriminator(hop_lengths=[15], hidden_channels=[32], domain='cepstral')
    with pytest.raises(ValueError, match='cepstral'):
        Discriminator(dict(hop_lengths=[15], hidden_channels=[32], domain='cepstral'), dict(_mrdcases.MPD))
    for domain, cin in (('double', 2), ('linear', 1), ('log', 1)):
        m = MultiResolutionDiscriminator(hop_lengths=[15], hidden_channels=[32], domain=domain)
        assert m.discriminators[0].discriminator[0]._modules['1'].weight_v.shape[1] == cin
