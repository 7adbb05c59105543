"""Waveform preparation on the gfx950 kernels (csrc/resample.hip): downmix, resample, peak-normalise -- step 1 of every recipe of
the reference (examples/csmsc/scripts/audio/audio_normalization.sh: ``sox in.wav -c 1 -r $sample_rate --norm=-7 out.wav``), which
stands before ``FeatureExtractor`` and ``PitchExtractor``.  sox's ``rate`` filter and its dither are not reproduced: the resampler
is a Kaiser-windowed-sinc polyphase filter, defined in csrc/resample.hip; the default design is resampy's published
``kaiser_best`` parameter set (the filter older ``librosa.load`` used), ``kaiser_fast`` is offered as well.

``polyphase_bank(up, down, zeros, rolloff, beta)`` -> ``(bank fp32 [up, P], half)``: the prototype filter in float64, rounded to
fp32 once, row p holding the taps of OUTPUT phase p.  ``Resampler(rate_in, rate_out, preset=..., zeros=, rolloff=, beta=,
device=)``: ``out_length(n) = ceil(n up / down)`` and ``resample(wav, lengths=None, norm_db=None) -> (out [B, L_out] fp32,
out_lengths [B] int64)``; ``wav`` is ``[B, L]``, ``[B, L, C]``, ``[L]`` or a list of ``[L]`` / ``[L, C]`` arrays or tensors, fp32
(float64 is rounded) or int16, which is uploaded as int16 and scaled on the device.  Channels are averaged; the samples behind an
utterance's ``L_out`` are 0.  ONE launch (``msmc_resample``) for the batch; with ``norm_db`` a second one (``msmc_peak_scale``)
scales every utterance so that its peak is ``10^(norm_db / 20)``, the peak taken AFTER the filter, which can raise it; a silent
utterance stays as it is.  ``rate_in == rate_out`` is the one-tap identity bank: a pure downmix.  The bank is built once per
device and kept on the instance.  Pairs are accepted up to ``up, down <= 1024`` and ``P <= 1024`` taps per phase; others raise.

``prepare_waveforms(wav, lengths, rate_in, rate_out, norm_db=-7.0, ...)`` is the reference's whole step 1 and returns what
``FeatureExtractor.extract`` and ``PitchExtractor.extract`` take, so the chain stays on the device.

Not here: sox's own filter and dither, sample formats other than those ``datasets/readers.py`` reads, and streaming of files too
long for one launch.  There is no CPU path: host tensors raise (``lib.ptr``) unless the tests' interpreter build is bound."""
import math

import numpy as np
import torch

from . import lib

PRESETS = {
    'kaiser_best': dict(zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492),
    'kaiser_fast': dict(zeros=16, rolloff=0.85, beta=8.555504641634386),
}
MAX_RATIO = 1024
MAX_TAPS = 1024
MAX_CHANNELS = 8


def ratio(rate_in, rate_out):
    """(up, down) in lowest terms"""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError('sample rates %d -> %d: both at least 1' % (rate_in, rate_out))
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def prototype_filter(up, down, zeros, rolloff, beta):
    """(h float64 [2 half + 1], half): h[k + half] = up fc sinc(fc k) kaiser(2 half + 1, beta)[k + half], fc = rolloff / max(up, down)"""
    mx = max(up, down)
    half = int(math.ceil(zeros * mx / rolloff))
    fc = rolloff / mx
    k = np.arange(-half, half + 1, dtype=np.float64)
    return up * fc * np.sinc(fc * k) * np.kaiser(2 * half + 1, beta), half


def polyphase_bank(up, down, zeros, rolloff, beta):
    """(bank fp32 [up, P], half): bank[p][j] = h[up j + (p down + half) % up - half], zero past the filter's end, so that
    y[q up + p] = sum_j bank[p][j] x[q down + (p down + half) // up - j]"""
    h, half = prototype_filter(up, down, zeros, rolloff, beta)
    P = -(-(2 * half + 1) // up)
    padded = np.zeros(up * P, dtype=np.float64)
    padded[:2 * half + 1] = h
    phases = (np.arange(up, dtype=np.int64) * down + half) % up
    bank = padded.reshape(P, up).T[phases]
    return np.ascontiguousarray(bank, dtype=np.float32), half


def batch_channels(wav, lengths, device=None):
    """-> (x [B, L, C] fp32 or int16, contiguous, on ``device`` -- for a list without one: the first CUDA item's device, else the
    current GPU --, host list of lengths)"""
    def as_pcm(x):
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype == torch.float64:
            return x.to(torch.float32)
        if x.dtype not in (torch.float32, torch.int16):
            raise TypeError('waveforms are fp32, float64 or int16, got %s' % x.dtype)
        return x

    if isinstance(wav, (list, tuple)):
        rows = [as_pcm(x) for x in wav]
        if not rows:
            raise ValueError('no waveforms')
        rows = [r.unsqueeze(-1) if r.dim() == 1 else r for r in rows]
        if any(r.dim() != 2 for r in rows):
            raise ValueError('a list holds [L] or [L, C] waveforms')
        if len(set((r.dtype, r.shape[1]) for r in rows)) != 1:
            raise ValueError('the waveforms of a batch share one dtype and one channel count')
        lens = [int(r.shape[0]) for r in rows]
        if lengths is not None and [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()] != lens:
            raise ValueError('lengths %s do not match the waveforms %s' % (list(lengths), lens))
        batch = torch.zeros((len(rows), max(max(lens), 1), rows[0].shape[1]), dtype=rows[0].dtype)
        for i, r in enumerate(rows):
            batch[i, :lens[i]] = r.cpu()
        dev = device if device is not None else next((r.device for r in rows if r.is_cuda), 'cuda')
        return batch.to(dev), lens
    wav = as_pcm(wav)
    if wav.dim() == 1:
        wav = wav.unsqueeze(0)
    if wav.dim() == 2:
        wav = wav.unsqueeze(-1)
    if wav.dim() != 3:
        raise ValueError('wav: expected [B, L], [B, L, C] or [L], got %s' % (tuple(wav.shape),))
    B, L = wav.shape[:2]
    lens = [L] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
    if len(lens) != B:
        raise ValueError('%d lengths for %d waveforms' % (len(lens), B))
    if any(n > L or n < 0 for n in lens):
        raise ValueError('lengths %d .. %d in a batch %d samples wide' % (min(lens), max(lens), L))
    if device is not None:
        wav = wav.to(device)
    return wav.contiguous(), lens


class Resampler(object):
    def __init__(self, rate_in, rate_out, preset='kaiser_best', zeros=None, rolloff=None, beta=None, device=None):
        if preset not in PRESETS:
            raise ValueError('preset %r: one of %s' % (preset, ', '.join(sorted(PRESETS))))
        self.rate_in, self.rate_out, self.preset = int(rate_in), int(rate_out), preset
        self.up, self.down = ratio(rate_in, rate_out)
        design = PRESETS[preset]
        self.zeros = int(design['zeros'] if zeros is None else zeros)
        self.rolloff = float(design['rolloff'] if rolloff is None else rolloff)
        self.beta = float(design['beta'] if beta is None else beta)
        if self.zeros < 1 or not 0 < self.rolloff <= 1 or self.beta < 0:
            raise ValueError('zeros = %d, rolloff = %g, beta = %g: zeros >= 1, 0 < rolloff <= 1, beta >= 0'
                             % (self.zeros, self.rolloff, self.beta))
        if self.up == self.down:                         # the same rate: the identity tap, a pure downmix
            self.half, self.taps = 0, 1
        else:
            self.half = int(math.ceil(self.zeros * max(self.up, self.down) / self.rolloff))
            self.taps = -(-(2 * self.half + 1) // self.up)
        if self.up > MAX_RATIO or self.down > MAX_RATIO or self.taps > MAX_TAPS:
            raise ValueError('%d -> %d Hz is %d / %d with %d taps per phase: the kernel takes up, down <= %d and at most %d taps'
                             % (self.rate_in, self.rate_out, self.up, self.down, self.taps, MAX_RATIO, MAX_TAPS))
        self.device = device
        self._bank = None
        self._consts = {}

    def out_length(self, n):
        """ceil(n up / down), in Python integers"""
        return -(-int(n) * self.up // self.down)

    def bank(self):
        """the fp32 bank [up, P] on the host"""
        if self._bank is None:
            if self.up == self.down:
                self._bank = np.ones((1, 1), dtype=np.float32)
            else:
                self._bank = polyphase_bank(self.up, self.down, self.zeros, self.rolloff, self.beta)[0]
            assert self._bank.shape == (self.up, self.taps)
        return self._bank

    def consts(self, device):
        """the bank on ``device``"""
        key = str(device)
        if key not in self._consts:
            self._consts[key] = torch.from_numpy(self.bank()).to(device)
        return self._consts[key]

    def resample(self, wav, lengths=None, norm_db=None, peak=False):
        """-> (out [B, L_out] fp32, out_lengths [B] int64); with ``peak`` also the peaks [B] before the scaling (``norm_db`` set)"""
        x, lens = batch_channels(wav, lengths, self.device)
        B, L, C = x.shape
        if C < 1 or C > MAX_CHANNELS:
            raise ValueError('%d channels: the kernel takes 1 .. %d' % (C, MAX_CHANNELS))
        if peak and norm_db is None:
            raise ValueError('the peaks are those of the normalisation: give norm_db')
        outs = [self.out_length(n) for n in lens]
        Lo = max(self.out_length(L), 1)
        if Lo >= 2 ** 31 - 2 ** 21:
            raise ValueError('%d output samples in one launch: fewer than 2^31 - 2^21' % Lo)
        h = lib.get()
        parts = h.msmc_resample_parts(Lo, self.up, self.down, self.taps)
        if parts < 1:
            raise ValueError('%d / %d with %d taps per phase is refused by the kernel' % (self.up, self.down, self.taps))
        with torch.no_grad():
            bank = self.consts(x.device)
            ln = torch.tensor(lens, dtype=torch.int32).to(x.device)
            y = torch.empty((B, Lo), dtype=torch.float32, device=x.device)
            part = torch.empty((B, parts), dtype=torch.float32, device=x.device)
            lib.call('msmc_resample', lib.ptr(x), int(x.dtype == torch.int16), lib.ptr(ln, torch.int32), lib.ptr(bank, torch.float32),
                     lib.ptr(y), lib.ptr(part), B, L, C, Lo, self.up, self.down, self.taps, self.half, lib.stream(x))
            pk = None
            if norm_db is not None:
                target = float(np.float32(10.0 ** (float(norm_db) / 20.0)))
                lo = torch.tensor(outs, dtype=torch.int32).to(x.device)
                pk = torch.empty((B,), dtype=torch.float32, device=x.device) if peak else None
                lib.call('msmc_peak_scale', lib.ptr(y), lib.ptr(part), lib.ptr(lo, torch.int32), lib.ptr(pk), B, Lo, parts, target,
                         lib.stream(x))
        if max(outs) < Lo:
            y = y[:, :max(max(outs), 1)].contiguous()
        out_lengths = torch.tensor(outs, dtype=torch.int64).to(x.device)
        return (y, pk, out_lengths) if peak else (y, out_lengths)


def prepare_waveforms(wav, lengths, rate_in, rate_out, norm_db=-7.0, preset='kaiser_best', device=None, resampler=None, **design):
    """the reference's step 1 (``sox -c 1 -r rate_out --norm=norm_db``): downmix, resample, then peak-normalise ->
    (out [B, L_out] fp32 on the device, out_lengths [B] int64), what ``FeatureExtractor.extract`` / ``PitchExtractor.extract``
    take as ``(wav, lengths)``.  ``resampler``: a ``Resampler`` for these rates to reuse (its bank is built once)."""
    rs = resampler if resampler is not None else Resampler(rate_in, rate_out, preset=preset, device=device, **design)
    if (rs.rate_in, rs.rate_out) != (int(rate_in), int(rate_out)):
        raise ValueError('a resampler for %d -> %d Hz given for %d -> %d Hz' % (rs.rate_in, rs.rate_out, rate_in, rate_out))
    return rs.resample(wav, lengths, norm_db=norm_db)
