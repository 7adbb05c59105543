"""GPU (-m gpu): the single-channel spectral domains of the resolution discriminators (``mrd_config.domain`` 'linear' / 'log')
over the real gfx950 library: the reference's own scores, feature maps and gradients (tests/golden/small_mrd_domains.npz), bit
equality with the two-channel image, the lock-step front-ends, front-end reuse, and one GAN-phase train step per domain eagerly,
replayed from hipGraphs and in bf16.  Cases and bounds: tests/_mrdcases.py."""
import math

import pytest
import torch

import _mrdcases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, L = 3, 2410


@pytest.fixture(scope='module', autouse=True)
def real_library():
    from msmctts_amd.hip import lib
    assert lib.backend() == 'gfx950', 'GPU tests must run on the real HIP library'
    torch.backends.cuda.matmul.allow_tf32 = False
    yield


@pytest.fixture(scope='module')
def waveform():
    return _mrdcases.t(_mrdcases.fixture()['wav']).to(DEV)


@pytest.mark.parametrize('domain,mel_scale', _mrdcases.CASES, ids=['%s-%s' % (d, 'mel' if m else 'plain') for d, m in _mrdcases.CASES])
def test_scores_feature_maps_and_gradients_match_the_reference(domain, mel_scale):
    """scores and every feature map within 1e-3 abs of the reference; the gradients of sum(score^2) with respect to the
    waveform and to each stack's first convolution at the gradient bar of the discriminator fixture (tests/_parity.py
    check_train_steps: norm within 2e-3, elements within 1e-5 + 2e-3 |reference|); B = 3, L = 2410, hops 15 / 50 / 240"""
    _mrdcases.check_fixture_case(DEV, domain, mel_scale)


def test_single_channel_image_is_that_channel_of_the_two_channel_image_bit_for_bit(waveform):
    assert tuple(waveform.shape) == (B, L)
    _mrdcases.check_image_exact(DEV, waveform, (15, 240))


def test_single_channel_image_backward_matches_autograd_across_both_clamp_edges():
    _mrdcases.check_image_backward(DEV)


def test_single_channel_image_unaligned_operands_and_refusals():
    _mrdcases.check_image_unaligned_and_refusals(DEV)


def test_front_ends_in_lock_step_equal_the_chains_one_by_one_for_every_domain(waveform):
    _mrdcases.check_lockstep(DEV, waveform, (15, 50, 240))


def test_front_end_reuse_gives_the_bits_of_a_fresh_front_end():
    _mrdcases.check_front_reuse(DEV, B=B, L=L, domain='log')


@pytest.fixture(scope='module')
def eager_losses():
    """the fp32 eager GAN-phase step of each domain: computed once, compared against by the graphed and the bf16 step"""
    cache = {}

    def get(domain):
        if domain not in cache:
            cache[domain] = _mrdcases.gan_step_losses(DEV, domain, graphed=False, amp_dtype=None)
        return cache[domain]
    return get


@pytest.mark.parametrize('domain', ['linear', 'log'])
def test_gan_step_replayed_from_graphs_matches_eager(domain, eager_losses):
    """tolerance of tests/test_gpu_parity.py test_graphed_step_matches_eager: 2e-3 max(1, |loss|) per loss"""
    e = eager_losses(domain)
    g = _mrdcases.gan_step_losses(DEV, domain, graphed=True, amp_dtype=None)
    print('eager  ', e)
    print('graphed', g)
    assert set(e) == set(g) and all(math.isfinite(v) for v in e.values())
    for k in e:
        assert abs(e[k] - g[k]) <= 2e-3 * max(1.0, abs(e[k])), (domain, k, e[k], g[k])


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
@pytest.mark.parametrize('domain', ['linear', 'log'])
def test_gan_step_in_bf16_is_finite_and_near_the_fp32_step(domain, graphed, eager_losses):
    """first-step bf16 bound of tests/test_gpu_fullsize.py (test_config2_bf16_graphed_grouped_step_trains): every loss within 2 %
    of the fp32 step's, relative to max(|fp32 loss|, 1e-2)"""
    e = eager_losses(domain)
    b = _mrdcases.gan_step_losses(DEV, domain, graphed=graphed, amp_dtype=torch.bfloat16)
    print('fp32', e)
    print('bf16', b)
    assert set(e) == set(b)
    for k in e:
        assert math.isfinite(b[k]), (domain, k, b[k])
        assert abs(b[k] - e[k]) / max(abs(e[k]), 1e-2) <= 0.02, (domain, k, b[k], e[k])
