"""Spectrogram and mel back to waveform on the gfx950 kernels (csrc/griffin_lim.hip): the linear spectrogram and the Griffin-Lim
inverses of the reference's examples/csmsc/scripts/audio/audio.py (``spectrogram``, ``inv_spectrogram``, ``fast_inv_spectrogram``,
``inv_mel_spectrogram`` with ``inv_preemphasis``, ``_mel_to_linear``, ``_denormalize``, ``_db_to_amp``, ``_stft`` / ``_istft``), which
the reference runs per file on librosa: how one listens to a mel -- from the feature files, from ``mel_outputs`` of the frame
decoder, from a predictor whose vocoder is not trained yet -- without a HifiGAN checkpoint.

``GriffinLim(**hparams, griffin_lim_iters=60, power=1.5)`` takes the reference's hparam names and defaults; the geometry, the
windowed DFT basis and the mel basis are those of its ``FeatureExtractor`` (``self.features``; hip/features.py).  Everything is
batched and ragged as ``extract`` is: ``[B, T, ...]`` with ``feat_length [B]`` frames per utterance, an utterance's result
independent of the rest of the batch.

    stft(wav, lengths)         -> (complex64 [B, T, F], feat_length)      librosa.stft as the reference calls it (no pre-emphasis)
    istft(spec, feat_length)   -> (wav [B, hop (T - 1)] fp32, lengths)    librosa.istft as the reference calls it
    spectrogram(wav, lengths)  -> (fp32 [B, T, F] normalised dB, feat_length)                           audio.spectrogram
    inv_spectrogram / fast_inv_spectrogram(spec [B, T, F], feat_length, phase=None, seed=0, iters=None)
    inv_mel_spectrogram(mel [B, T, M], feat_length, phase=None, seed=0, iters=None, fast=False)
                               -> (wav [B, hop (T - 1)] fp32, lengths [B] int64) on the device

The initial phases are ``phase`` ([B, T, F], in turns, what ``np.random.rand`` gives the reference) or drawn on the host from
``seed``: utterance b takes ``RandomState(seed + b).rand(F, T_b)``, so a seeded utterance does not depend on its batch either.

THE ONE-OFF PREPARATION KEEPS STOCK OPERATORS, a stated choice: ``_denormalize``, ``_db_to_amp``, ``_mel_to_linear`` (the
pseudo-inverse of the mel basis by ``np.linalg.pinv`` in float64 on the host, once per instance; the 1e-10 floor), ``** power`` and
``S exp(2 pi i u)`` are torch operators on the device in float64, rounded to fp32 once.  They run once against the iterations, and
the magnitudes stay exact enough that the tests need no allowance for them.  Each ITERATION is exactly two launches -- ``msmc_stft``
in its projection mode (the spectrum of the current waveform, projected onto the magnitudes, with the ``alpha = 0.99`` momentum of
``_fast_griffin_lim`` where asked), then ``msmc_istft`` -- and ``msmc_deemphasis`` runs once at the end; nothing is read back
during the loop.  An utterance with ``hop (T_b - 1) <= n_fft / 2`` samples is refused before any launch: the iteration's reflect
padding needs more.

There is no CPU path: host tensors raise (``lib.ptr``) unless the tests' interpreter build is bound.  Forward only."""
import numpy as np
import torch

from . import lib
from .features import HPARAMS, FeatureExtractor

MODE_COMPLEX, MODE_PROJECT, MODE_DB = 0, 1, 2
FAST_ALPHA = 0.99


def inverse_dft_basis(n_fft, win, fq, ks):
    """[ceil(win / fq), KP, fq] float32, KP = 2 F rounded up to whole ``ks``: row k < F holds c_f w[n] cos(2 pi f (n + off) / n_fft)
    / n_fft for f = k, row F + f holds -c_f w[n] sin(...) / n_fft; c_f = 1 for DC and Nyquist (whose sine rows are zero, as irfft
    ignores those imaginary parts), 2 otherwise; w periodic Hann of ``win`` samples, off = (n_fft - win) // 2.  Only the ``win``
    taps under the window exist; zero columns past them.  Built in float64."""
    F = n_fft // 2 + 1
    ntt, kp = -(-win // fq), -(-2 * F // ks) * ks
    n = np.arange(win, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n.astype(np.float64) / win)
    f = np.arange(F, dtype=np.int64)
    ang = 2.0 * np.pi * ((f[:, None] * (n[None, :] + (n_fft - win) // 2)) % n_fft).astype(np.float64) / n_fft
    cf = np.where((f == 0) | (f == n_fft // 2), 1.0, 2.0)[:, None]
    rows = np.zeros((kp, ntt * fq))
    rows[:F, :win] = cf * w[None, :] * np.cos(ang) / n_fft
    rows[F:2 * F, :win] = np.where(cf == 1.0, 0.0, -cf * w[None, :] * np.sin(ang) / n_fft)
    return np.ascontiguousarray(rows.reshape(kp, ntt, fq).transpose(1, 0, 2)).astype(np.float32)


def window_squares(win):
    """[win] float32: the squares of the periodic Hann window, float64 rounded once"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)
    return (w * w).astype(np.float32)


class GriffinLim(object):
    def __init__(self, griffin_lim_iters=60, power=1.5, device=None, **hparams):
        self.features = FeatureExtractor(device=device, **hparams)
        self.griffin_lim_iters, self.power = int(griffin_lim_iters), float(power)
        if self.griffin_lim_iters < 0:
            raise ValueError('griffin_lim_iters = %d: not negative' % self.griffin_lim_iters)
        fe = self.features
        self.n_fft, self.hop, self.win, self.num_freq = fe.n_fft, fe.hop, fe.win, fe.n_fft // 2 + 1
        self.device = device
        self._inv_mel = None
        self._consts = {}

    @classmethod
    def from_config(cls, conf, **kw):
        """as ``FeatureExtractor.from_config``; the mapping may also name ``griffin_lim_iters`` and ``power``"""
        conf = dict(conf.get('hparams', conf) or {})
        return cls(**dict({k: conf[k] for k in HPARAMS + ('griffin_lim_iters', 'power') if k in conf}, **kw))

    def inv_mel_basis(self):
        """[F, M] float64: ``np.linalg.pinv`` of the extractor's mel basis, once per instance"""
        if self._inv_mel is None:
            self._inv_mel = np.linalg.pinv(self.features._mel_basis.astype(np.float64))
        return self._inv_mel

    def consts(self, device):
        """(ibasis, wsq, inverse mel basis [F, M] float64) on ``device`` (``msmc_istft`` of include/msmc_hip.h)"""
        key = str(device)
        if key not in self._consts:
            h = lib.get()
            if h.msmc_istft_tile(self.n_fft, self.win, self.hop) < 1:
                raise ValueError('n_fft %d, window %d, hop %d: the inverse transform takes ceil(win / hop) <= 32 and a window of '
                                 'at most 1118 samples' % (self.n_fft, self.win, self.hop))
            ib = inverse_dft_basis(self.n_fft, self.win, h.msmc_stft_tile(1), h.msmc_stft_tile(2))
            self._consts[key] = (torch.from_numpy(ib).to(device), torch.from_numpy(window_squares(self.win)).to(device),
                                 torch.from_numpy(self.inv_mel_basis()).to(device))
        return self._consts[key]

    # ---- the three launches ---------------------------------------------------------------------------------------------------
    def _stft(self, x, ln, T, mode, out, mag=None, prev=None, alpha=0.0, preemphasis=0.0):
        fe = self.features
        basis = fe.consts(x.device)[0]
        lib.call('msmc_stft', lib.ptr(x, torch.float32), lib.ptr(ln, torch.int32), lib.ptr(basis), mode, lib.ptr(out, torch.float32),
                 lib.ptr(mag, torch.float32), lib.ptr(prev, torch.float32), alpha, x.shape[0], x.shape[1], T, self.n_fft, self.win,
                 self.hop, preemphasis, fe.ref_level_db, fe.min_level_db, fe.max_abs_value, int(fe.symmetric_specs), lib.stream(x))

    def _istft(self, spec, frames, y):
        ib, wsq, _ = self.consts(spec.device)
        lib.call('msmc_istft', lib.ptr(spec, torch.float32), lib.ptr(frames, torch.int32), lib.ptr(ib), lib.ptr(wsq),
                 lib.ptr(y, torch.float32), spec.shape[0], spec.shape[1], self.n_fft, self.win, self.hop, lib.stream(spec))

    def _forward(self, wav, lengths, mode, preemphasis):
        x, lens = self.features._batch(wav, lengths)
        for n in lens:
            if n <= self.n_fft // 2:
                raise ValueError('an utterance of %d samples: reflect padding needs more than n_fft / 2 = %d' % (n, self.n_fft // 2))
        B, T, F = x.shape[0], self.features.feat_length(max(lens)), self.num_freq
        with torch.no_grad():
            ln = torch.tensor(lens, dtype=torch.int32).to(x.device)
            out = torch.empty((B, T, F) if mode == MODE_DB else (B, T, 2, F), dtype=torch.float32, device=x.device)
            self._stft(x, ln, T, mode, out, preemphasis=preemphasis)
        return out, torch.tensor([self.features.feat_length(n) for n in lens], dtype=torch.int64).to(x.device)

    def stft(self, wav, lengths=None, planar=False):
        """what ``extract`` takes -> (complex64 [B, T, F] -- with ``planar`` the kernel's fp32 [B, T, 2, F]: per frame the real
        parts, then the imaginary parts --, feat_length [B] int64); zero rows behind each utterance's frames"""
        out, feat_length = self._forward(wav, lengths, MODE_COMPLEX, 0.0)
        return (out if planar else torch.complex(out[:, :, 0], out[:, :, 1])), feat_length

    def spectrogram(self, wav, lengths=None):
        """``audio.spectrogram``: (normalised dB magnitudes [B, T, F] fp32, feat_length [B] int64)"""
        return self._forward(wav, lengths, MODE_DB, self.features.preemphasis)

    def _frames(self, feat_length, B, T):
        lens = [T] * B if feat_length is None else [int(v) for v in torch.as_tensor(feat_length).reshape(-1).tolist()]
        if len(lens) != B or any(n < 1 or n > T for n in lens):
            raise ValueError('feat_length %s for a batch of %d utterances of %d frames' % (lens, B, T))
        return lens

    def _planar(self, spec):
        if torch.is_complex(spec):
            spec = torch.stack([spec.real, spec.imag], dim=2)
        if spec.dim() != 4 or spec.shape[2] != 2 or spec.shape[3] != self.num_freq or spec.shape[1] < 2:
            raise ValueError('spec: expected complex [B, T >= 2, %d] or planar [B, T, 2, %d], got %s'
                             % (self.num_freq, self.num_freq, tuple(spec.shape)))
        return spec.to(torch.float32).contiguous()

    def istft(self, spec, feat_length=None):
        """spec: complex [B, T, F] or planar fp32 [B, T, 2, F] -> (wav [B, hop (T - 1)] fp32, lengths [B] int64 = hop (T_b - 1))"""
        spec = spec if torch.is_tensor(spec) else torch.from_numpy(np.ascontiguousarray(spec))
        if self.device is not None:
            spec = spec.to(self.device)
        spec = self._planar(spec)
        lens = self._frames(feat_length, spec.shape[0], spec.shape[1])
        with torch.no_grad():
            fr = torch.tensor(lens, dtype=torch.int32).to(spec.device)
            y = torch.empty((spec.shape[0], self.hop * (spec.shape[1] - 1)), dtype=torch.float32, device=spec.device)
            self._istft(spec, fr, y)
        return y, torch.tensor([self.hop * (n - 1) for n in lens], dtype=torch.int64).to(spec.device)

    def deemphasis(self, wav, lengths, out=None):
        """``inv_preemphasis`` of a padded batch [B, L] fp32 (in place unless ``out``), up to each length"""
        out = wav if out is None else out
        ln = torch.as_tensor(lengths).to(torch.int32).to(wav.device)
        lib.call('msmc_deemphasis', lib.ptr(wav, torch.float32), lib.ptr(out, torch.float32), lib.ptr(ln, torch.int32), wav.shape[0],
                 wav.shape[1], self.features.preemphasis, lib.stream(wav))
        return out

    # ---- the preparation (stock operators, float64) and the loop --------------------------------------------------------------
    def _features_in(self, x, width, feat_length):
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[2] != width:
            raise ValueError('expected [B, T, %d] or [T, %d], got %s' % (width, width, tuple(x.shape)))
        x = (x if self.device is None else x.to(self.device)).contiguous()
        lens = self._frames(feat_length, x.shape[0], x.shape[1])
        for n in lens:
            if self.hop * (n - 1) <= self.n_fft // 2:
                raise ValueError('an utterance of %d frames gives %d samples: the iteration\'s reflect padding needs more than '
                                 'n_fft / 2 = %d' % (n, self.hop * (n - 1), self.n_fft // 2))
        lib.ptr(x)                                         # (a host tensor without the interpreter raises before any work)
        return x, lens

    def amplitudes(self, x, mel=False):
        """``_db_to_amp(_denormalize(x) + ref_level_db)`` -- for a mel then ``_mel_to_linear`` -- ``** power``: float64 [B, T, F]"""
        fe = self.features
        x = x.to(torch.float64)
        lo, top = fe.min_level_db, fe.max_abs_value
        if fe.symmetric_specs:
            D = (torch.clamp(x, -top, top) + top) * -lo / (2 * top) + lo
        else:
            D = torch.clamp(x, 0, top) * -lo / top + lo
        A = torch.pow(10.0, (D + fe.ref_level_db) * 0.05)
        if mel:
            A = torch.clamp(A @ self.consts(x.device)[2].T, min=1e-10)
        return A ** self.power

    def initial_phases(self, lens, T, seed):
        """[B, T, F] float64 in turns: utterance b draws ``RandomState(seed + b).rand(F, T_b)``, zero rows behind"""
        u = np.zeros((len(lens), T, self.num_freq))
        for b, n in enumerate(lens):
            u[b, :n] = np.random.RandomState(int(seed) + b).rand(self.num_freq, n).T
        return torch.from_numpy(u)

    def griffin_lim(self, S, lens, phase=None, seed=0, iters=None, fast=False, deemphasis=True):
        """S: float64 magnitudes [B, T, F] on the device -> (wav, lengths): ``_griffin_lim`` / ``_fast_griffin_lim`` and, unless
        told otherwise, ``inv_preemphasis``"""
        iters = self.griffin_lim_iters if iters is None else int(iters)
        B, T, F = S.shape
        dev = S.device
        with torch.no_grad():
            u = self.initial_phases(lens, T, seed) if phase is None else torch.as_tensor(phase)
            if tuple(u.shape) != (B, T, F):
                raise ValueError('phase: expected %s, got %s' % ((B, T, F), tuple(u.shape)))
            u = (2.0 * np.pi) * u.to(torch.float64).to(dev)
            c = torch.stack([S * torch.cos(u), S * torch.sin(u)], dim=2).to(torch.float32).contiguous()
            mag = S.to(torch.float32).contiguous()
            prev = c.clone() if fast else None
            fr = torch.tensor(lens, dtype=torch.int32).to(dev)
            ln = torch.tensor([self.hop * (n - 1) for n in lens], dtype=torch.int32).to(dev)
            y = torch.empty((B, self.hop * (T - 1)), dtype=torch.float32, device=dev)
            self._istft(c, fr, y)
            for _ in range(iters):
                self._stft(y, ln, T, MODE_PROJECT, c, mag=mag, prev=prev, alpha=FAST_ALPHA if fast else 0.0)
                self._istft(c, fr, y)
            if deemphasis:
                self.deemphasis(y, ln)
        return y, ln.to(torch.int64)

    def inv_spectrogram(self, spec, feat_length=None, phase=None, seed=0, iters=None, fast=False):
        """normalised dB spectrogram [B, T, F] (what ``spectrogram`` returns) -> (wav [B, hop (T - 1)] fp32, lengths [B] int64)"""
        x, lens = self._features_in(spec, self.num_freq, feat_length)
        return self.griffin_lim(self.amplitudes(x), lens, phase, seed, iters, fast)

    def fast_inv_spectrogram(self, spec, feat_length=None, phase=None, seed=0, iters=None):
        return self.inv_spectrogram(spec, feat_length, phase, seed, iters, fast=True)

    def inv_mel_spectrogram(self, mel, feat_length=None, phase=None, seed=0, iters=None, fast=False):
        """normalised mel [B, T, M] (what ``extract`` returns) -> (wav [B, hop (T - 1)] fp32, lengths [B] int64)"""
        x, lens = self._features_in(mel, self.features.num_mels, feat_length)
        return self.griffin_lim(self.amplitudes(x, mel=True), lens, phase, seed, iters, fast)


def save_wav_pcm(wav):
    """the reference's ``save_wav`` scaling: float -> int16 with the peak at 32767 (peaks below 0.01 are not raised further)"""
    wav = np.asarray(wav, dtype=np.float64)
    peak = np.max(np.abs(wav)) if wav.size else 0.0
    return (wav * (32767 / max(0.01, peak))).astype(np.int16)
