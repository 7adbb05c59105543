"""Acoustic features from waveforms on the gfx950 kernel (csrc/features.hip): the ``mel/<id>.npy`` and ``energy/<id>.npy`` files
every recipe of the reference starts from (examples/csmsc/scripts/audio/melspectrogram.py -> audio.py ``melspectrogram`` /
``energy``: pre-emphasis, ``librosa.stft(center=True)``, magnitude, Slaney mel, dB, normalise and clip; the l2 norm of a frame's
magnitudes), which the reference computes in a CPU process pool on librosa.

``FeatureExtractor(...)`` takes the hparams of the reference's hparams.py under their names and defaults; the geometry follows
``_stft_parameters`` (``n_fft = 2 (num_freq - 1)``, ``hop`` / ``win`` = ``int(ms / 1000 * sample_rate)``; ``hop_length`` /
``win_length`` override the two for geometries no millisecond value yields).  ``extract(wav, lengths=None, energy=True)`` ->
``(mel [B, T, M], energy [B, T] or None, feat_length [B])`` with ``T = 1 + max(lengths) // hop`` and zero rows behind each
utterance's ``1 + L // hop`` frames: ONE launch (``msmc_mel_features``) for the batch, every utterance reflect-padded at its own
length, its rows independent of the rest of the batch.  The window is folded into the DFT basis (float64, rounded to fp32 once);
the mel basis is ``mel_filterbank`` of trainers/criterions/stft_loss.py, the one ``MelLoss`` uses.  Both constants are built once
per device and kept on the instance.

There is no CPU path: host tensors raise (``lib.ptr``) unless the tests' interpreter build is bound.  Forward only."""
import numpy as np
import torch

from . import lib

MAX_MELS = 128

HPARAMS = ('sample_rate', 'num_mels', 'num_freq', 'frame_length_ms', 'frame_shift_ms', 'preemphasis', 'min_level_db',
           'ref_level_db', 'max_abs_value', 'symmetric_specs')


def windowed_dft_basis(n_fft, win, fq, ks):
    """[ceil(F / fq), WP, 2 fq] float32: for frequency tile j and tap n, w[n] cos(2 pi (n + off) f / n_fft) for the tile's fq
    frequencies, then -w[n] sin(...); w periodic Hann of ``win`` samples, off = (n_fft - win) // 2 (the window centred in n_fft);
    zero rows up to WP = win rounded up to whole ``ks``, zero columns past F = n_fft // 2 + 1.  Built in float64."""
    F = n_fft // 2 + 1
    nft, wp = -(-F // fq), -(-win // ks) * ks
    n = np.arange(win, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n.astype(np.float64) / win)
    f = np.arange(nft * fq, dtype=np.int64)
    ang = 2.0 * np.pi * (((n[:, None] + (n_fft - win) // 2) * f[None, :]) % n_fft).astype(np.float64) / n_fft
    live = (f < F)[None, :]
    cos = np.where(live, w[:, None] * np.cos(ang), 0.0).reshape(win, nft, fq)
    sin = np.where(live, -w[:, None] * np.sin(ang), 0.0).reshape(win, nft, fq)
    out = np.zeros((nft, wp, 2 * fq), dtype=np.float32)
    out[:, :win, :fq] = cos.transpose(1, 0, 2)
    out[:, :win, fq:] = sin.transpose(1, 0, 2)
    return out


def energy_track(energy):
    """[B, T] -> [B, T, 1]: the ``energy`` entry of a batch as ``synthetic.make_emb_batch(tracks=True)`` lays it out"""
    return energy.unsqueeze(-1)


def batch_waveforms(wav, lengths, device=None):
    """a [B, L] or [L] tensor / array, or a list of 1-D waveforms -> (fp32 [B, L] tensor on ``device`` -- for a list without one:
    the first CUDA row's device, else the current GPU --, host list of lengths); integer PCM is scaled to [-1, 1) as the wav
    readers do.  Shared by ``FeatureExtractor`` and ``PitchExtractor`` (hip/pitch.py)."""
    def as_f32(x):
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype == torch.int16:
            return x.to(torch.float32) / 32768.0
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError('waveforms are fp32, float64 or int16, got %s' % x.dtype)
        return x.to(torch.float32)

    if isinstance(wav, (list, tuple)):
        rows = [as_f32(x).reshape(-1) for x in wav]
        if not rows:
            raise ValueError('no waveforms')
        lens = [int(r.numel()) for r in rows]
        batch = torch.zeros((len(rows), max(lens)), dtype=torch.float32)
        for i, r in enumerate(rows):
            batch[i, :lens[i]] = r.cpu()
        if lengths is not None and [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()] != lens:
            raise ValueError('lengths %s do not match the waveforms %s' % (list(lengths), lens))
        dev = device if device is not None else next((r.device for r in rows if r.is_cuda), 'cuda')
        return batch.to(dev), lens
    wav = wav if torch.is_tensor(wav) else torch.from_numpy(np.ascontiguousarray(wav))
    if wav.dim() == 1:
        wav = wav.unsqueeze(0)
    if wav.dim() != 2:
        raise ValueError('wav: expected [B, L] or [L], got %s' % (tuple(wav.shape),))
    B, L = wav.shape
    lens = [L] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
    if len(lens) != B:
        raise ValueError('%d lengths for %d waveforms' % (len(lens), B))
    if any(n > L for n in lens):
        raise ValueError('a length of %d in a batch %d samples wide' % (max(lens), L))
    wav = as_f32(wav)
    if device is not None:
        wav = wav.to(device)
    return wav.contiguous(), lens


class FeatureExtractor(object):
    def __init__(self, sample_rate=16000, num_mels=80, num_freq=1025, frame_length_ms=50, frame_shift_ms=12.5, preemphasis=0.97,
                 min_level_db=-100, ref_level_db=20, max_abs_value=4.0, symmetric_specs=True, win_length=None, hop_length=None,
                 device=None):
        self.sample_rate, self.num_mels, self.num_freq = int(sample_rate), int(num_mels), int(num_freq)
        self.frame_length_ms, self.frame_shift_ms = frame_length_ms, frame_shift_ms
        self.preemphasis, self.min_level_db, self.ref_level_db = float(preemphasis), float(min_level_db), float(ref_level_db)
        self.max_abs_value, self.symmetric_specs = float(max_abs_value), bool(symmetric_specs)
        self.n_fft = (self.num_freq - 1) * 2
        self.hop = int(frame_shift_ms / 1000 * sample_rate) if hop_length is None else int(hop_length)
        self.win = int(frame_length_ms / 1000 * sample_rate) if win_length is None else int(win_length)
        if self.num_mels < 1 or self.num_mels > MAX_MELS:
            raise ValueError('num_mels = %d: the kernel takes 1 .. %d mel bins' % (self.num_mels, MAX_MELS))
        if self.n_fft < 2:
            raise ValueError('num_freq = %d: at least 2 frequency bins' % self.num_freq)
        if self.win < 1 or self.win > self.n_fft:
            raise ValueError('window of %d samples: 1 .. n_fft = %d' % (self.win, self.n_fft))
        if self.hop < 1:
            raise ValueError('hop of %d samples: at least 1' % self.hop)
        if not self.min_level_db < 0 or not self.max_abs_value > 0:
            raise ValueError('min_level_db = %g must be negative, max_abs_value = %g positive' % (self.min_level_db, self.max_abs_value))
        self.device = device
        from ..trainers.criterions.stft_loss import mel_filterbank       # (the trainers import this package)
        self._mel_basis = mel_filterbank(self.sample_rate, self.n_fft, self.num_mels, 0, self.sample_rate / 2.0)   # [M, F] fp32
        self._consts = {}

    @classmethod
    def from_config(cls, conf, **kw):
        """from a mapping that names some of the hparams (the reference's hparams.py as a yaml file); the rest keep their defaults"""
        conf = dict(conf.get('hparams', conf) or {})
        return cls(**dict({k: conf[k] for k in HPARAMS if k in conf}, **kw))

    def feat_length(self, n_samples):
        return 1 + n_samples // self.hop

    def consts(self, device):
        """(basis, melT) on ``device``, in the kernel's tiling (``msmc_mel_features`` of include/msmc_hip.h)"""
        key = str(device)
        if key not in self._consts:
            tile = lib.get().msmc_mel_features_tile
            fq, ks = tile(1), tile(2)
            basis = windowed_dft_basis(self.n_fft, self.win, fq, ks)
            F, M = self.n_fft // 2 + 1, self.num_mels
            melT = np.zeros((basis.shape[0] * fq, -(-M // 32) * 32), dtype=np.float32)
            melT[:F, :M] = self._mel_basis.T
            self._consts[key] = (torch.from_numpy(basis).to(device), torch.from_numpy(melT).to(device))
        return self._consts[key]

    def _batch(self, wav, lengths):
        return batch_waveforms(wav, lengths, self.device)

    def extract(self, wav, lengths=None, energy=True, energy_track=False):
        """wav: [B, L] or [L] tensor / array, or a list of 1-D arrays / tensors (padded on the host, uploaded once) ->
        (mel [B, T, M], energy [B, T] -- [B, T, 1] with ``energy_track`` -- or None, feat_length [B] int64)"""
        x, lens = self._batch(wav, lengths)
        for n in lens:
            if n <= self.n_fft // 2:
                raise ValueError('an utterance of %d samples: reflect padding needs more than n_fft / 2 = %d' % (n, self.n_fft // 2))
        B, L = x.shape
        T = self.feat_length(max(lens))
        with torch.no_grad():
            basis, melT = self.consts(x.device)
            ln = torch.tensor(lens, dtype=torch.int32).to(x.device)
            mel = torch.empty((B, T, self.num_mels), dtype=torch.float32, device=x.device)
            en = torch.empty((B, T), dtype=torch.float32, device=x.device) if energy else None
            lib.call('msmc_mel_features', lib.ptr(x, torch.float32), lib.ptr(ln, torch.int32), lib.ptr(basis), lib.ptr(melT),
                     lib.ptr(mel), lib.ptr(en), B, L, T, self.n_fft, self.win, self.hop, self.num_mels, self.preemphasis,
                     self.ref_level_db, self.min_level_db, self.max_abs_value, int(self.symmetric_specs), lib.stream(x))
        feat_length = torch.tensor([self.feat_length(n) for n in lens], dtype=torch.int64).to(x.device)
        if en is not None and energy_track:
            en = en.unsqueeze(-1)
        return mel, en, feat_length
