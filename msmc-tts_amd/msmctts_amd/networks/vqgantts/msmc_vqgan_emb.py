"""MSMC-VQ-GAN over self-supervised speech embeddings -- the QS-TTS synthesiser (drop-in for reference
msmctts/networks/vqgantts/msmc_vqgan_emb.py:14-291; configuration examples/qs-tts/configs/synthesizer/
msmc_vq_gan_hubertch_aishell3.yaml: 1024-dimensional HuBERT frames in, 16 kHz waveform out).

Same classes, constructor kwargs, ``state_dict`` keys and output dictionaries as the reference.  The reference file imports
a module that is not in its tree (``msmc_vqgan_speech``, :11); by its use of ``ResStack`` and ``MultiStageQuantizer`` it is
the MSMC-VQ-GAN module under another name, which is what this file builds on: the multi-stage
quantiser (gfx950 VQ kernels, 1x1 stacks and prior predictor on the implicit-GEMM kernels), the FFT-block stacks and the
HifiGAN generator are the ones of ``msmc_vqgan.py``.  New here: ``MAMSEncoder`` (the multi-stage encoder with an optional
pitch / energy side encoder added to every stage's output) and the optional reference-encoder slot.

The speaker / style reference encoder (``global_encoder_config._name == 'ECAPA_TDNN'``, reference :143-151) is ``tdnn.py``'s
``ECAPA_TDNN(in_channels=mel_dim, embd_dim=n_model_size, channels=n_model_size)`` on the gfx950 kernels: its utterance-level
embedding of ``ref`` (training: of ``mel`` when no ``ref`` is given) is added to every frame of the frame decoder's input
(:195-199, :254-258).  Sizes its kernels do not take (``n_model_size % 64``, ``mel_dim % 8``) are refused at construction with
``NotImplementedError``; an unknown encoder name raises ``ValueError`` as in the reference.

``KMeansQuantizer`` / ``KMeansVQGANEmb`` (reference :294-469) are the discrete-unit baseline: the embedding frames themselves are
snapped to the centroids of a frozen, offline k-means model (one head of emb_dim channels, any number of centroids: the search
runs ``msmc_vq_search_wide``, csrc/vq_wide.inc, where the other search kernels refuse the shape), then pass through ``in_linear``,
the optional global encoder and frame decoder and the vocoder.  Same class names, constructor keywords, ``state_dict`` keys
(``quantizer.quantizer.0.{embed,cluster_size,embed_avg}``, ``in_linear``, ``decoder``, ``frame_decoder``, ``global_encoder``,
``mel_predictor``) and output-dictionary keys (``encoder_indices``, ``mel_outputs``, ``decoder_outputs``); ``forward`` takes the
``window`` / ``window_frames`` forms of ``MSMCVQGANEmb.forward``.  ``quantizer_path`` is a pickle holding an object with
``cluster_centers_`` [K, d] as in the reference (unpickling a scikit-learn model needs scikit-learn installed; nothing here
imports it) or, in addition, a ``.npy`` file of shape [K, d] -- which ``fit_kmeans`` (hip/kmeans.py, exported here: Lloyd's
algorithm on the gfx950 kernels) produces from frames [N, d].  The step between fitting and training -- frames to units -- is
``assign_units`` / ``collapse_units`` / ``unit_usage`` / ``usage_summary`` (hip/units.py, exported here too) and
``KMeansQuantizer.units``: labels only, through ``msmc_vq_assign_wide``.  Deviations from the reference:

* the reference assigns ``embed`` from the file at every forward (:316), so a checkpoint's ``embed`` never counts.  Here the
  centroids are copied into the buffer at construction and again after every ``load_state_dict``: the same observable result;
* the reference's training-mode ``analysis`` unpacks the quantiser's dictionary with ``zip(*...)`` (:429) and cannot work; here it
  raises ``NotImplementedError`` naming that line;
* ``synthesis`` hands the quantiser a ``zip`` the reference's quantiser has consumed by the time it lists the lengths (:329, :440),
  so its ``quantizer_lengths`` come out empty; nothing reads them there, and here they are the lengths given;
* sizes the downstream kernels refuse (``n_model_size % 64``, ``mel_dim % 8`` with a global encoder) raise at construction, as
  for ``MSMCVQGANEmb``.

The unit-input path (no reference counterpart): ``forward_units`` / ``synthesis_units`` take the stored labels [B, T] (or runs,
through ``expand_units``) in the place of embedding frames.  With a frozen codebook ``in_linear(embed_code(ind))`` is a row of
``unit_table() = centers W^T + b`` [K, n_model_size], so the decoder input is ``unit_embed`` (csrc/unit_embed.hip): one gather
that also adds the global embedding, and for the gradient a per-label sum followed by the table's small GEMM -- no upload of
frames, no nearest-centroid search, no ``in_linear`` over the frames.  Deviation from the frame path: padded rows (and rows whose
label is outside [0, K)) of the decoder input are zeros there, where the frame path has whatever ``in_linear`` makes of the
padding frames; the FFT blocks mask padded positions, so with a frame decoder the valid frames do not see the difference.

The stage in front of the units (no reference counterpart either): ``KMeansVQGANEmb.compute_embedding_loss`` is the loss of a
text -> unit predictor against this model (``trainers/unit_predictor_trainer.py``) -- ``'softmax'`` over the K centroids on
csrc/unit_ce.hip, ``'mse'`` and the ``'triple*'`` methods as for the multi-stage quantiser -- and ``decode_units`` turns such a
predictor's logits into the labels (or runs) ``synthesis_units`` takes.

The stored-code path of the main model (no reference counterpart): ``MSMCVQGANEmb.analysis_codes`` / ``synthesis_codes`` take the
``quantizer_indices`` a run of ``analysis`` produced (``tools/extract_codes.py`` stores them) in the place of frames and rebuild
the per-stage ``quantizer_outputs`` with one gather per stage (csrc/code_embed.hip) -- what ``EmbPredictorTrainer`` trains a text
front-end on without running the frozen encoder and search at every step.  Deviation from ``analysis``: that returns the search
kernel's straight-through value ``o = x + (q - x)`` (csrc/vq_common.inc: x the quantiser's input, q the code row), which is
the code row up to two fp32 roundings; ``analysis_codes`` returns the code row q itself.  In fp32
``|o - q| <= 2^-24 (|x| + 2 |q|)`` element by element (the rounding of q - x is at most 2^-24 (|q| + |x|), that of the sum at
most 2^-24 |o| ~ 2^-24 |q|).
"""
import pickle

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...hip import losses as hiploss
from ...hip import norm as hipnorm
from ...hip import side_enc as hipside
from ...hip import unit_ce as hipunitce
from ...hip import window as hipwindow
from ...hip.kmeans import fit_kmeans, kmeans_plusplus  # noqa: F401  -- fits the file ``KMeansQuantizer`` loads (``fit_kmeans(...).save(path)``)
from ...hip.features import FeatureExtractor  # noqa: F401  -- waveforms -> the mel / energy files the datasets read (hip/features.py)
from ...hip.griffin_lim import GriffinLim  # noqa: F401  -- and back: spectrogram / mel -> waveform by Griffin-Lim (hip/griffin_lim.py)
from ...hip.pitch import PitchExtractor  # noqa: F401  -- waveforms -> the pitch files, on the same frame grid (hip/pitch.py)
from ...hip.resample import Resampler, prepare_waveforms  # noqa: F401  -- downmix, resample, peak-normalise before the two (hip/resample.py)
from ...hip import units as hipunits
from ...hip import vq as hipvq
from ...hip.units import assign_units, collapse_units, unit_usage, usage_summary  # noqa: F401  -- frames -> units on that file
from ...hip.units import expand_units, unit_embed  # noqa: F401  -- and units -> the decoder input (``forward_units``)
from ...hip.convnet import ConvBank, ConvLayer, hip_conv
from ...utils.utils import get_mask_from_lengths
from ..acoustic_models.transformer import FFTBlocks
from ..hifigan.generator import Generator as HifiGANGenerator
from .modules import Quantize
from .msmc_vqgan import MultiStageQuantizer, PriorPredictor, _fft_pos
from .tdnn import ECAPA_TDNN


class AttrPredictor(PriorPredictor):
    """reference msmc_vqgan_emb.py:14-38: the prior predictor's WaveNet stack + 1x1 projection under another name"""


class MAMSEncoder(nn.Module):
    """multi-stage FFT-block encoder (reference :41-120): stage i average-pools the previous stage's output by
    ``downsample_scales[i]``; when pitch / energy tracks are given their encoding (a small Conv1d / Tanh stack, pooled
    alongside) is ADDED to every stage's output -- after the first stage's output has been set aside as the content
    representation"""

    def __init__(self, in_channels, pitch_dim=1, energy_dim=1, downsample_scales=[1], max_seq_len=2400, n_layers=4, n_head=2,
                 d_k=64, d_v=64, d_inner=1024, fft_conv1d_kernel=3, fft_conv1d_padding=1, dropout=0.2, attn_dropout=0.1,
                 fused_layernorm=False):
        super().__init__()
        self.downsample_scales = list(downsample_scales)
        self.encoders = nn.ModuleList([
            FFTBlocks(max_seq_len=max_seq_len, n_layers=n_layers, n_head=n_head, d_k=d_k, d_v=d_v, d_model=in_channels,
                      d_inner=d_inner, fft_conv1d_kernel=fft_conv1d_kernel, fft_conv1d_padding=fft_conv1d_padding,
                      dropout=dropout, attn_dropout=attn_dropout, fused_layernorm=fused_layernorm, name='encoder_%d' % i)
            for i in range(len(self.downsample_scales))])
        self.use_pitch = pitch_dim + energy_dim > 0
        if self.use_pitch:
            self.pitch_encoder = nn.Sequential(
                nn.Conv1d(pitch_dim + energy_dim, in_channels, 7, padding=3), nn.Tanh(),
                nn.Conv1d(in_channels, in_channels, 3, padding=1), nn.Tanh(),
                nn.Conv1d(in_channels, in_channels, 3, padding=1), nn.Tanh(),
                nn.Conv1d(in_channels, in_channels, 1))

    # True: the side encoder runs on csrc/side_enc.hip (first layer + Tanh, pooling + addition) and the implicit-GEMM kernels (the
    # three C -> C layers) wherever they take the operands; False on an instance keeps the stock chain (tests and the bench compare)
    fused_side = True

    def _side_bank(self):
        """the three C -> C layers of the side encoder as plain layers of one small ConvBank (fp32, as the side encoder computes);
        None where the convolution kernels refuse the width -- those layers then stay on stock operators"""
        if not hasattr(self, '_mid'):
            self._mid = None
            mods = [self.pitch_encoder[i] for i in (2, 4, 6)]
            if all(m.in_channels % 8 == 0 and m.out_channels % 8 == 0 for m in mods):
                layers = [ConvLayer(m, 'conv', (1, m.kernel_size[0]), (1, 1), (1, 1), (0, m.padding[0]), plain=True) for m in mods]
                self._mid = (ConvBank(layers), layers)
        if self._mid is not None:
            self._mid[0].prepare(torch.float32)
        return self._mid

    def _side_fused(self, pitch, energy):
        """the side encoding [B, T, C] fp32, channels-last, or None where the kernels do not take the operands"""
        if not self.fused_side:
            return None
        first = self.pitch_encoder[0]
        width = lambda t: 0 if t is None else t.shape[-1]
        if width(pitch) + width(energy) != first.in_channels or not hipside.front_usable(
                pitch if width(pitch) else None, energy if width(energy) else None, first.weight):
            return None
        side = hipside.side_front(pitch, energy, first.weight, first.bias)
        mid = self._side_bank()
        if mid is None:
            side = side.transpose(1, 2)
            for m in list(self.pitch_encoder)[2:]:
                side = m(side)
            return side.transpose(1, 2).contiguous()
        bank, layers = mid
        for i, layer in enumerate(layers):
            side = hip_conv(bank, layer, side.unsqueeze(1)).squeeze(1)
            if i < 2:
                side = hipnorm.tanh(side.contiguous())
        return side

    def forward(self, emb, input_length, pitch=None, energy=None):
        fused = False
        if self.use_pitch:
            side = self._side_fused(pitch, energy)
            fused = side is not None
            if not fused:
                side = self.pitch_encoder(torch.cat((pitch, energy), dim=-1).transpose(1, 2).float()).transpose(1, 2)
        outputs, content = [], None
        feat, flen = emb, input_length
        for enc, scale in zip(self.encoders, self.downsample_scales):
            if scale > 1:
                feat = F.avg_pool1d(feat.transpose(1, 2), kernel_size=scale, stride=scale, ceil_mode=True).transpose(1, 2)
                if self.use_pitch and not fused:
                    side = F.avg_pool1d(side.transpose(1, 2), kernel_size=scale, stride=scale, ceil_mode=True).transpose(1, 2)
                flen = torch.ceil(flen / scale).int()
            feat, _ = enc(feat, _fft_pos(flen, feat), lengths=flen)
            if not outputs:
                content = feat
            if self.use_pitch:
                if fused and hipside.pool_usable(side, feat, scale):
                    side, feat = hipside.pool_add(side, feat, scale)       # (pooled for the next stage, stage output + pooled)
                else:
                    if fused and scale > 1:
                        side = F.avg_pool1d(side.transpose(1, 2), kernel_size=scale, stride=scale, ceil_mode=True).transpose(1, 2)
                    feat = feat + side.to(feat.dtype)
            outputs.append((feat, flen))
        return outputs, content


class MSMCVQGANEmb(nn.Module):
    def __init__(self, emb_dim, n_model_size, pitch_dim=1, energy_dim=1, encoder_config=None, quantizer_config=None,
                 global_encoder_config=None, frame_decoder_config=None, decoder_config=None, pred_mel=False, mel_dim=None):
        super().__init__()
        self.in_linear = nn.Linear(emb_dim, n_model_size)
        self.encoder = MAMSEncoder(n_model_size, pitch_dim=pitch_dim, energy_dim=energy_dim, **encoder_config)
        if global_encoder_config is not None:
            name = (global_encoder_config.get('_name') if isinstance(global_encoder_config, dict)
                    else getattr(global_encoder_config, '_name', None))
            if name != 'ECAPA_TDNN':
                raise ValueError('Wrong global encoder: {}'.format(name))
            self.global_encoder = ECAPA_TDNN(in_channels=mel_dim, embd_dim=n_model_size, channels=n_model_size)
        self.quantizer = MultiStageQuantizer(n_model_size, list(encoder_config['downsample_scales'])[::-1],
                                             **quantizer_config)
        decoder_config = dict(decoder_config)
        decoder_config['num_mels'] = n_model_size
        self.decoder = HifiGANGenerator(**decoder_config)
        if frame_decoder_config is not None:
            self.frame_decoder = FFTBlocks(d_model=n_model_size, name='frame_decoder', **frame_decoder_config)
        if pred_mel:
            self.mel_predictor = nn.Linear(n_model_size, mel_dim if mel_dim is not None else emb_dim)

    def _decode_frames(self, x, lengths, ref=None):
        if hasattr(self, 'global_encoder'):
            x = x + self.global_encoder(ref).unsqueeze(1).to(x.dtype)
        return self._frame_decode(x, lengths)

    def _frame_decode(self, x, lengths):
        """the half of ``_decode_frames`` behind the global embedding (``KMeansVQGANEmb.forward_units`` adds that in its kernel)"""
        if hasattr(self, 'frame_decoder'):
            x, _ = self.frame_decoder(x, _fft_pos(lengths, x), lengths=lengths)
        return x

    def _window(self, dec_in, window, window_frames):
        """the vocoder's input frames for ``window`` (see ``forward``).  On the GPU (or with the interpreter build bound) the
        (utterance, start) table and the reference's triples of equal length run hip/window.py's ``window_gather``: one launch
        into the generator's compute dtype and channels-last layout, one launch for the gradient -- the same values as the
        slice / stack / cast chain, which every other form keeps"""
        if window_frames is not None:
            if not (torch.is_tensor(window) and window.dim() == 2 and window.shape[1] == 2 and window.dtype == torch.int32):
                raise TypeError('window_frames goes with an int32 [n, 2] tensor of (utterance, start) pairs')
            return hipwindow.window_gather(dec_in, window, int(window_frames), self.decoder.hip_dtype)
        if torch.is_tensor(window):
            return torch.gather(dec_in, 1, window.unsqueeze(-1).expand(-1, -1, dec_in.shape[-1]))
        if isinstance(window, (list, tuple)):
            if hipwindow.usable(dec_in) and len(window) > 0:
                B, T = dec_in.shape[:2]
                W = window[0][2] - window[0][1]
                us = [i for i, _, _ in window]
                if (W >= 1 and all(0 <= i < B and 0 <= s and e - s == W and e <= T for i, s, e in window)
                        and all(b > a for a, b in zip(us, us[1:]))):
                    return hipwindow.window_gather(dec_in, [(i, s) for i, s, _ in window], W, self.decoder.hip_dtype)
            return torch.stack([dec_in[i, s:e] for i, s, e in window], dim=0)
        return dec_in

    def forward(self, emb, emb_length, pitch=None, energy=None, mel=None, ref=None, window='full', window_frames=None):
        """``window``: None = no waveform (frames only), 'full' = decode every frame, a list of (utterance, start, end)
        frame triples (the reference's convention here, :206-209) or a [B, n] tensor of frame indices = decode those; with
        ``window_frames`` = W, an int32 [n, 2] device tensor of (utterance, start) pairs = decode W frames from each start
        (strictly increasing utterance indices; frames past the end read as zeros)"""
        if self.training:
            hipnorm.advance_seed(emb.device)        # fresh dropout masks for the fused kernels of this step
        enc, content = self.encoder(self.in_linear(emb), emb_length, pitch, energy)
        feats, lens = zip(*enc)
        qs = self.quantizer(enc)
        out = {'encoder_outputs': feats[::-1], 'encoder_lengths': lens[::-1], 'content_representations': content,
               'encoder_indices': qs['quantizer_indices'], 'encoder_diffs': qs['quantizer_diffs'],
               'decoder_diffs': qs['predictor_diffs']}
        dec_in = self._decode_frames(qs['residual_output'], emb_length, mel if ref is None else ref)
        if hasattr(self, 'mel_predictor'):
            out['mel_outputs'] = self.mel_predictor(dec_in)
        if window is not None:
            dec_in = self._window(dec_in, window, window_frames)
            out['decoder_outputs'] = self.decoder(dec_in.transpose(1, 2)).transpose(1, 2)
        return out

    def analysis(self, emb, emb_length, pitch=None, energy=None):
        enc, content = self.encoder(self.in_linear(emb), emb_length, pitch, energy)
        qs = self.quantizer(enc)
        if self.training:
            feats, lens = zip(*enc)
            return {'encoder_outputs': feats[::-1], 'encoder_lengths': lens[::-1],
                    'encoder_indices': qs['quantizer_indices'], 'encoder_diffs': qs['quantizer_diffs'],
                    'decoder_diffs': qs['predictor_diffs'], 'quantizer_states': qs, 'content_representations': content}
        return qs

    def analysis_codes(self, indices, lengths):
        """What eval-mode ``analysis`` returns that a predictor step reads -- ``quantizer_outputs``, ``quantizer_indices``,
        ``quantizer_lengths`` -- from the stored ``quantizer_indices`` (per stage, coarse to fine) and the per-stage lengths:
        ``MultiStageQuantizer.embed_codes``, one gather per stage; no frames, no encoder, no search.  Eval mode only (the codebook
        must be the one the indices were extracted with): ``RuntimeError`` in training mode."""
        if self.training:
            raise RuntimeError('analysis_codes needs a frozen codebook: call it in eval mode')
        return self.quantizer.embed_codes(indices, lengths)

    def synthesis(self, quantizer_outputs, quantizer_lengths, ref=None):
        qs = quantizer_outputs
        if not isinstance(quantizer_outputs, dict):
            qs = self.quantizer(zip(quantizer_outputs, quantizer_lengths), from_encoder=False)
        if hasattr(self, 'global_encoder'):
            assert ref is not None
        dec_in = self._decode_frames(qs['residual_output'], quantizer_lengths[-1], ref)
        wav = self.decoder(dec_in.transpose(1, 2)).transpose(1, 2)
        if self.training:
            out = {'decoder_outputs': wav}
            if hasattr(self, 'mel_predictor'):
                out['mel_outputs'] = self.mel_predictor(dec_in)
            return out
        return wav

    def synthesis_codes(self, indices, lengths, ref=None):
        """``synthesis`` from stored code indices: the waveform of ``analysis_codes(indices, lengths)['quantizer_outputs']``"""
        return self.synthesis(self.analysis_codes(indices, lengths)['quantizer_outputs'], lengths, ref)

    def compute_embedding_loss(self, quantizer_outputs, quantizer_lengths, quantizer_states, methods=['mse'],
                               loss_weights=[1.0]):
        states = [{'predictor_outputs': quantizer_outputs[i],
                   'target_outputs': quantizer_states['quantizer_outputs'][i],
                   'target_indices': quantizer_states['quantizer_indices'][i],
                   'target_lengths': quantizer_lengths[i]} for i in range(len(quantizer_outputs))]
        return self.quantizer.compute_embedding_loss(states, methods, loss_weights)


class EmbVC(nn.Module):
    """the quantiser-free voice-conversion model (reference :472-628): ``in_linear`` -> ``MAMSEncoder`` (pitch / energy side
    encoder added to every stage) -> + the global encoder's utterance embedding of ``ref`` (training: of ``mel``) -> frame decoder ->
    optional ``mel_predictor`` -> HifiGAN, the decoder input being the LAST stage's output as it is.  Constructor keywords,
    ``state_dict`` keys and output-dictionary keys (``encoder_outputs``, ``encoder_lengths``, ``content_representations``,
    ``mel_outputs``, ``decoder_outputs``) are the reference's; ``forward`` also takes the ``window`` / ``window_frames`` forms of
    ``MSMCVQGANEmb.forward``; the size refusals are ``MSMCVQGANEmb``'s.  The last stage must run at the input's frame rate
    (``downsample_scales`` all 1 in the reference's use), or the global embedding, the frame decoder's positions and the windows
    would not line up -- as in the reference.
    The reference's ``analysis``, ``synthesis`` and ``compute_embedding_loss`` use a ``self.quantizer`` the class never creates
    (:568, :587, :628) and cannot run; here they raise ``NotImplementedError`` naming the line."""

    def __init__(self, emb_dim, n_model_size, pitch_dim=1, energy_dim=1, encoder_config=None, global_encoder_config=None,
                 frame_decoder_config=None, decoder_config=None, pred_mel=False, mel_dim=None):
        super().__init__()
        self.in_linear = nn.Linear(emb_dim, n_model_size)
        self.encoder = MAMSEncoder(n_model_size, pitch_dim=pitch_dim, energy_dim=energy_dim, **encoder_config)
        if global_encoder_config is not None:
            name = (global_encoder_config.get('_name') if isinstance(global_encoder_config, dict)
                    else getattr(global_encoder_config, '_name', None))
            if name != 'ECAPA_TDNN':
                raise ValueError('Wrong global encoder: {}'.format(name))
            self.global_encoder = ECAPA_TDNN(in_channels=mel_dim, embd_dim=n_model_size, channels=n_model_size)
        decoder_config = dict(decoder_config)
        decoder_config['num_mels'] = n_model_size
        self.decoder = HifiGANGenerator(**decoder_config)
        if frame_decoder_config is not None:
            self.frame_decoder = FFTBlocks(d_model=n_model_size, name='frame_decoder', **frame_decoder_config)
        if pred_mel:
            self.mel_predictor = nn.Linear(n_model_size, mel_dim if mel_dim is not None else emb_dim)

    _decode_frames = MSMCVQGANEmb._decode_frames
    _frame_decode = MSMCVQGANEmb._frame_decode
    _window = MSMCVQGANEmb._window

    def forward(self, emb, emb_length, pitch=None, energy=None, mel=None, ref=None, window='full', window_frames=None):
        """``window`` / ``window_frames`` as ``MSMCVQGANEmb.forward``"""
        if self.training:
            hipnorm.advance_seed(emb.device)
        enc, content = self.encoder(self.in_linear(emb), emb_length, pitch, energy)
        feats, lens = zip(*enc)
        out = {'encoder_outputs': feats[::-1], 'encoder_lengths': lens[::-1], 'content_representations': content}
        dec_in = self._decode_frames(feats[-1], emb_length, mel if ref is None else ref)
        if hasattr(self, 'mel_predictor'):
            out['mel_outputs'] = self.mel_predictor(dec_in)
        if window is not None:
            dec_in = self._window(dec_in, window, window_frames)
            out['decoder_outputs'] = self.decoder(dec_in.transpose(1, 2)).transpose(1, 2)
        return out

    def analysis(self, emb, emb_length, pitch=None, energy=None):
        raise NotImplementedError('EmbVC.analysis: the reference quantises with a self.quantizer the class never creates '
                                  '(msmc_vqgan_emb.py:568) and cannot run; forward() returns the encoder outputs')

    def synthesis(self, quantizer_outputs, quantizer_lengths, ref=None):
        raise NotImplementedError('EmbVC.synthesis: the reference quantises with a self.quantizer the class never creates '
                                  '(msmc_vqgan_emb.py:587) and cannot run; forward() decodes to the waveform')

    def compute_embedding_loss(self, quantizer_outputs, quantizer_lengths, quantizer_states, methods=['mse'], loss_weights=[1.0]):
        raise NotImplementedError('EmbVC.compute_embedding_loss: the reference calls a self.quantizer the class never creates '
                                  '(msmc_vqgan_emb.py:628) and cannot run')


def _load_centroids(path):
    """[K, d] float32 from a ``.npy`` file or a pickled object with ``cluster_centers_`` (reference :297-300)"""
    if str(path).endswith('.npy'):
        centers = np.load(path, allow_pickle=False)
    else:
        with open(path, 'rb') as fin:
            centers = pickle.load(fin).cluster_centers_
    centers = torch.as_tensor(np.asarray(centers), dtype=torch.float32)
    if centers.dim() != 2 or centers.shape[0] < 1 or centers.shape[1] < 1:
        raise ValueError('%s: expected centroids of shape [K, d], got %s' % (path, tuple(centers.shape)))
    return centers


class KMeansQuantizer(nn.Module):
    """one frozen ``Quantize`` over the centroids of an offline k-means model (reference :294-336); only ever searched with
    ``update=False``"""

    def __init__(self, model_path):
        super().__init__()
        codewords = _load_centroids(model_path).t().contiguous()                 # [d, K], the layout of ``Quantize.embed``
        self.register_buffer('codewords', codewords, persistent=False)           # (not a ``state_dict`` key, as in the reference)
        self.quantizer = nn.ModuleList([Quantize(codewords.shape[0], codewords.shape[1])])
        self._restore()
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._restore())

    def _restore(self):
        with torch.no_grad():
            self.quantizer[0].embed.copy_(self.codewords)

    def forward(self, encoder_states, from_encoder=True):
        encoder_states = list(encoder_states)
        states = [self.quantizer[i](embedding, length, update=False) for i, (embedding, length) in enumerate(encoder_states)]
        outputs, diffs, indices = zip(*states)
        return {'residual_output': None, 'quantizer_outputs': outputs, 'quantizer_diffs': diffs, 'quantizer_indices': indices,
                'quantizer_lengths': [length for _, length in encoder_states], 'predictor_diffs': None}

    def units(self, emb, emb_length, collapse=False):
        """emb [B, T, d] -> labels [B, T] int64 without quant and diff (``msmc_vq_assign_wide`` on this module's centroids, no
        gradient): the ``quantizer_indices`` of ``forward`` wherever that runs the wide search -- every single head
        ``msmc_vq_search`` refuses, unit codebooks among them -- since the two kernels share the search.  ``collapse``: also the
        runs of the valid prefixes, ``(labels, units [B, T], dur [B, T] int32, ulen [B])`` (``collapse_units``)."""
        B, T, d = emb.shape
        with torch.no_grad():
            embed_t, enorm = hipvq.vq_prepare(self.quantizer[0].embed.unsqueeze(0), frames=0)
            labels, _ = hipunits.assign_wide(emb.detach().reshape(B * T, d).float(), embed_t, enorm, want_dist=False)
            labels = labels.view(B, T)
            if not collapse:
                return labels
            return (labels,) + hipunits.collapse_units(labels, emb_length)


class KMeansVQGANEmb(nn.Module):
    def __init__(self, emb_dim, n_model_size, quantizer_path, global_encoder_config=None, frame_decoder_config=None,
                 decoder_config=None, pred_mel=False, mel_dim=None):
        super().__init__()
        if global_encoder_config is not None:
            name = (global_encoder_config.get('_name') if isinstance(global_encoder_config, dict)
                    else getattr(global_encoder_config, '_name', None))
            if name != 'ECAPA_TDNN':
                raise ValueError('Wrong global encoder: {}'.format(name))
            self.global_encoder = ECAPA_TDNN(in_channels=mel_dim, embd_dim=n_model_size, channels=n_model_size)
        self.quantizer = KMeansQuantizer(quantizer_path)
        self.in_linear = nn.Linear(emb_dim, n_model_size)
        decoder_config = dict(decoder_config)
        decoder_config['num_mels'] = n_model_size
        self.decoder = HifiGANGenerator(**decoder_config)
        if frame_decoder_config is not None:
            self.frame_decoder = FFTBlocks(d_model=n_model_size, name='frame_decoder', **frame_decoder_config)
        if pred_mel:
            self.mel_predictor = nn.Linear(n_model_size, mel_dim if mel_dim is not None else emb_dim)

    _decode_frames = MSMCVQGANEmb._decode_frames
    _frame_decode = MSMCVQGANEmb._frame_decode
    _window = MSMCVQGANEmb._window

    def forward(self, emb, emb_length, pitch=None, energy=None, mel=None, ref=None, window='full', window_frames=None):
        """``window`` / ``window_frames`` as ``MSMCVQGANEmb.forward``; ``pitch`` / ``energy`` are accepted and unused, as in the
        reference (:380-383)"""
        if self.training:
            hipnorm.advance_seed(emb.device)
        qs = self.quantizer([(emb, emb_length)])
        out = {'encoder_indices': qs['quantizer_indices']}
        dec_in = self._decode_frames(self.in_linear(qs['quantizer_outputs'][-1]), emb_length, mel if ref is None else ref)
        if hasattr(self, 'mel_predictor'):
            out['mel_outputs'] = self.mel_predictor(dec_in)
        if window is not None:
            dec_in = self._window(dec_in, window, window_frames)
            out['decoder_outputs'] = self.decoder(dec_in.transpose(1, 2)).transpose(1, 2)
        return out

    def unit_table(self):
        """[K, n_model_size]: ``in_linear`` of every centroid, the rows ``forward_units`` gathers.  Differentiable in
        ``in_linear``; computed anew at every call (the weights move with every optimizer step)"""
        centers = self.quantizer.quantizer[0].embed.detach().t()
        return F.linear(centers, self.in_linear.weight, self.in_linear.bias)

    def _embed_units(self, ind, length, ref):
        glob = None
        if hasattr(self, 'global_encoder'):
            glob = self.global_encoder(ref).float()
        return unit_embed(ind, length, self.unit_table().float(), glob)

    def forward_units(self, ind, length, mel=None, ref=None, window='full', window_frames=None):
        """``forward`` from stored labels: ind [B, T] int64 (-1 or anything behind ``length``), length [B].  The dictionary of
        ``forward`` with ``encoder_indices = (ind,)``; ``window`` / ``window_frames`` as there.  The decoder input is
        ``unit_embed(ind, length, unit_table(), global embedding of ref or mel)``; the frame decoder, ``mel_predictor``, the
        window and the vocoder follow as in ``forward``."""
        if self.training:
            hipnorm.advance_seed(ind.device)
        out = {'encoder_indices': (ind,)}
        dec_in = self._frame_decode(self._embed_units(ind, length, mel if ref is None else ref), length)
        if hasattr(self, 'mel_predictor'):
            out['mel_outputs'] = self.mel_predictor(dec_in)
        if window is not None:
            dec_in = self._window(dec_in, window, window_frames)
            out['decoder_outputs'] = self.decoder(dec_in.transpose(1, 2)).transpose(1, 2)
        return out

    def synthesis_units(self, ind, length=None, *third, ref=None, dur=None, ulen=None):
        """``synthesis`` from stored labels.  Without ``dur``: ind [B, T] frame labels, ``length`` [B] (None: every frame).
        With ``dur`` [B, R]: ``ind`` holds the units of (unit, duration) runs, ``ulen`` [B] their number (None: every slot), and
        the frame labels come from ``expand_units`` (one read-back to size them).  Returns what ``synthesis`` returns.
        The runs also come positionally, ``synthesis_units(units, dur, ulen, ref=...)`` -- what ``decode_units(..., collapse=True)``
        and ``collapse_units`` return: a two-dimensional second argument is the durations.  (Otherwise a third positional
        argument is ``ref``, as it always was.)"""
        if len(third) > 1:
            raise TypeError('synthesis_units takes at most three positional arguments')
        if torch.is_tensor(length) and length.dim() == 2 and dur is None:
            dur, length = length, None
            if third:
                ulen = third[0]
        elif third:
            ref = third[0]
        if dur is not None:
            if ulen is None:
                ulen = torch.full((ind.shape[0],), ind.shape[1], dtype=torch.int64, device=ind.device)
            ind, length = expand_units(ind, dur, ulen)
        elif length is None:
            length = torch.full((ind.shape[0],), ind.shape[1], dtype=torch.int64, device=ind.device)
        if hasattr(self, 'global_encoder'):
            assert ref is not None
        dec_in = self._frame_decode(self._embed_units(ind, length, ref), length)
        wav = self.decoder(dec_in.transpose(1, 2)).transpose(1, 2)
        if self.training:
            out = {'decoder_outputs': wav}
            if hasattr(self, 'mel_predictor'):
                out['mel_outputs'] = self.mel_predictor(dec_in)
            return out
        return wav

    def compute_embedding_loss(self, quantizer_outputs, quantizer_lengths, quantizer_states, methods=['mse'],
                               loss_weights=[1.0]):
        """The losses of a predictor of this model's units (no reference counterpart; signature and keys of
        ``MSMCVQGANEmb.compute_embedding_loss``: ``embed_loss_<method>_0`` and ``total_loss``).  One stage: ``quantizer_outputs[0]``
        [B, T, width] is the prediction, ``quantizer_states['quantizer_indices'][0]`` [B, T] the unit labels (-1 allowed on
        padding), ``quantizer_lengths[0]`` the lengths.  Methods: ``'softmax'`` -- the prediction is logits whose first K columns
        are the K centroids (a projection may be built wider), ``masked_cross_entropy`` (csrc/unit_ce.hip), which also leaves the
        count of frames whose arg-max is the label in ``quantizer_states['unit_correct']`` (a 0-dim device tensor); ``'mse'`` -- against
        ``quantizer_states['quantizer_outputs'][0]``, or the centroid rows of the labels where the states carry none; the
        ``'triple*'`` methods -- ``Quantize.compute_triple_loss`` (the wide kernel at unit widths).  Every term is the masked sum over
        valid frames divided by the sum of the lengths."""
        q = self.quantizer.quantizer[0]
        p, lengths = quantizer_outputs[0], quantizer_lengths[0]
        ind = quantizer_states['quantizer_indices'][0].detach().reshape(p.shape[:2])
        weights = loss_weights[0] if isinstance(loss_weights[0], (list, tuple)) else loss_weights
        losses, parts, pweights = {}, [], []

        def masked(loss):
            loss = loss.masked_fill(get_mask_from_lengths(lengths.to(loss.device), loss.shape[1]), 0)
            return loss.sum() / lengths.sum()
        for method, weight in zip(methods, weights):
            if method == 'softmax':
                loss, correct = hipunitce.masked_cross_entropy(p, ind, lengths, classes=q.n_embed, return_correct=True)
                if isinstance(quantizer_states, dict):
                    quantizer_states['unit_correct'] = correct
            elif method == 'mse':
                frames = (quantizer_states.get('quantizer_outputs') or (None,))[0]
                if frames is None:
                    frames = q.embed_code(ind.clamp(0, q.n_embed - 1))
                frames = frames.detach()
                if (hiploss.usable(p) and p.dtype in (torch.float32, torch.bfloat16) and frames.dtype in (torch.float32, torch.bfloat16)
                        and lengths.device == p.device and lengths.dtype in (torch.int32, torch.int64)):
                    loss = hiploss.masked_mean(p, lengths, b=frames)
                else:
                    loss = masked(F.mse_loss(p, frames, reduction='none').mean(-1))
            elif method in ('triple', 'triple_mean', 'triple_sum'):
                # (a label outside [0, K) can only be padding: masked below, clamped so that the kernel reads a codeword)
                loss = masked(q.compute_triple_loss(p, ind.clamp(0, q.n_embed - 1), reduction='sum' if method == 'triple_sum' else 'mean'))
            else:
                raise NotImplementedError('embedding loss %r' % method)
            losses['embed_loss_%s_0' % method] = loss
            parts.append(loss)
            pweights.append(weight)
        losses['total_loss'] = hiploss.weighted_sum(parts, pweights) if parts else 0
        return losses

    def decode_units(self, logits, length, collapse=False):
        """A unit predictor's logits [B, T, width] (the first K columns are the K centroids) -> labels [B, T] int64, -1 behind
        ``length`` (``unit_argmax``, csrc/unit_ce.hip); ``collapse``: the runs ``(units, dur, ulen)`` of ``collapse_units``
        instead -- ``synthesis_units(*decode_units(logits, length, collapse=True), ref=...)`` is the waveform."""
        length = torch.as_tensor(length).to(device=logits.device)
        if length.dtype not in (torch.int32, torch.int64):
            length = length.long()
        labels = hipunitce.unit_argmax(logits, length, classes=self.quantizer.quantizer[0].n_embed)
        return collapse_units(labels, length) if collapse else labels

    def analysis(self, emb, emb_length):
        if self.training:
            raise NotImplementedError('KMeansVQGANEmb.analysis in training mode: the reference unpacks the quantiser\'s dictionary '
                                      'with zip(*...) there (msmc_vqgan_emb.py:429) and cannot run; call it in eval mode')
        return self.quantizer([(emb, emb_length)])

    def synthesis(self, quantizer_outputs, quantizer_lengths, ref=None):
        """the sequences are quantised again (reference :440): centroid rows map to themselves"""
        qs = self.quantizer(zip(quantizer_outputs, quantizer_lengths))
        if hasattr(self, 'global_encoder'):
            assert ref is not None
        dec_in = self._decode_frames(self.in_linear(qs['quantizer_outputs'][-1]), quantizer_lengths[-1], ref)
        wav = self.decoder(dec_in.transpose(1, 2)).transpose(1, 2)
        if self.training:
            out = {'decoder_outputs': wav}
            if hasattr(self, 'mel_predictor'):
                out['mel_outputs'] = self.mel_predictor(dec_in)
            return out
        return wav
