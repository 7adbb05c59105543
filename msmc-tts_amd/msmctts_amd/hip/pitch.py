"""F0 tracks from waveforms on the gfx950 kernel (csrc/pitch.hip): the ``pitch/<id>.npy`` files ``TTSDataset`` and ``EmbDataset``
read and the ``pitch`` entry the side encoder of ``EmbVC`` / ``MSMCVQGANEmb`` takes.  The reference ships no F0 tracker; it fixes
only the convention of the track (utils/audio.py ``lf02sinexi`` / ``lf02peakexi``: natural-log F0 on voiced frames, a value <= 0
on unvoiced ones).  The algorithm is YIN, steps 1-5 (de Cheveigne & Kawahara 2002), defined in csrc/pitch.hip.

``PitchExtractor(...)`` shares ``sample_rate``, ``frame_length_ms`` and ``frame_shift_ms`` (``win_length`` / ``hop_length``
override the two) with ``FeatureExtractor``, so the frame grid is the same -- ``T = 1 + L // hop``, frame t centred on sample
t hop -- and mel, energy and pitch line up row for row.  ``fmin`` / ``fmax`` bound the lags (``tau_min = sr // fmax``,
``tau_max = sr // fmin``), ``threshold`` is YIN's absolute threshold on the normalised difference; ``log=False`` gives Hz.
``extract(wav, lengths=None, voiced=False, aperiodicity=False, pitch_track=False)`` -> ``(pitch [B, T], ...the extras asked
for, in that order..., feat_length [B])``: ONE launch (``msmc_pitch_yin``) for the batch, every utterance reflect-padded at its own
length, its rows independent of the rest of the batch; unvoiced frames and the rows behind an utterance's frames are 0.

There is no CPU path: host tensors raise (``lib.ptr``) unless the tests' interpreter build is bound.  Forward only."""
import torch

from . import lib
from .features import batch_waveforms

HPARAMS = ('sample_rate', 'frame_length_ms', 'frame_shift_ms', 'fmin', 'fmax', 'threshold')


def pitch_track(pitch):
    """[B, T] -> [B, T, 1]: the ``pitch`` entry of a batch as ``synthetic.make_emb_batch(tracks=True)`` lays it out"""
    return pitch.unsqueeze(-1)


class PitchExtractor(object):
    def __init__(self, sample_rate=16000, frame_length_ms=50, frame_shift_ms=12.5, fmin=60, fmax=500, threshold=0.15, log=True,
                 win_length=None, hop_length=None, device=None):
        self.sample_rate = int(sample_rate)
        self.frame_length_ms, self.frame_shift_ms = frame_length_ms, frame_shift_ms
        self.fmin, self.fmax, self.threshold, self.log = fmin, fmax, float(threshold), bool(log)
        self.hop = int(frame_shift_ms / 1000 * sample_rate) if hop_length is None else int(hop_length)
        self.win = int(frame_length_ms / 1000 * sample_rate) if win_length is None else int(win_length)
        if self.sample_rate < 1:
            raise ValueError('sample_rate = %d: at least 1' % self.sample_rate)
        if not 0 < fmin < fmax:
            raise ValueError('fmin = %g, fmax = %g: 0 < fmin < fmax' % (fmin, fmax))
        self.tau_min, self.tau_max = int(self.sample_rate // fmax), int(self.sample_rate // fmin)
        if self.tau_min < 2:
            raise ValueError('fmax = %g at %d Hz: the shortest lag sr // fmax = %d must be at least 2 samples'
                             % (fmax, self.sample_rate, self.tau_min))
        if self.tau_max <= self.tau_min:
            raise ValueError('fmin = %g, fmax = %g at %d Hz: lags %d .. %d leave no range'
                             % (fmin, fmax, self.sample_rate, self.tau_min, self.tau_max))
        if not self.threshold > 0:
            raise ValueError('threshold = %g: must be positive' % self.threshold)
        if self.win < 1:
            raise ValueError('window of %d samples: at least 1' % self.win)
        if self.hop < 1:
            raise ValueError('hop of %d samples: at least 1' % self.hop)
        self.span = self.win + self.tau_max + 1
        self.device = device

    @classmethod
    def from_config(cls, conf, **kw):
        """from the mapping ``FeatureExtractor.from_config`` reads (hparams at the top level or under ``hparams``), which may also
        name ``fmin``, ``fmax`` and ``threshold``; the rest keep their defaults"""
        conf = dict(conf.get('hparams', conf) or {})
        return cls(**dict({k: conf[k] for k in HPARAMS if k in conf}, **kw))

    def feat_length(self, n_samples):
        return 1 + n_samples // self.hop

    def extract(self, wav, lengths=None, voiced=False, aperiodicity=False, pitch_track=False, cmnd=False):
        """wav: what ``FeatureExtractor.extract`` takes -> (pitch [B, T] -- [B, T, 1] with ``pitch_track`` --, then voiced [B, T]
        uint8, aperiodicity [B, T] and cmnd [B, T, tau_max + 2] (the normalised difference itself: for the tests) where asked
        for, feat_length [B] int64)"""
        x, lens = batch_waveforms(wav, lengths, self.device)
        for n in lens:
            if n <= self.span // 2:
                raise ValueError('an utterance of %d samples: reflect padding needs more than (win + tau_max + 1) // 2 = %d'
                                 % (n, self.span // 2))
        B, L = x.shape
        T = self.feat_length(max(lens))
        with torch.no_grad():
            ln = torch.tensor(lens, dtype=torch.int32).to(x.device)
            f0 = torch.empty((B, T), dtype=torch.float32, device=x.device)
            vo = torch.empty((B, T), dtype=torch.uint8, device=x.device) if voiced else None
            ap = torch.empty((B, T), dtype=torch.float32, device=x.device) if aperiodicity else None
            cm = torch.empty((B, T, self.tau_max + 2), dtype=torch.float32, device=x.device) if cmnd else None
            lib.call('msmc_pitch_yin', lib.ptr(x, torch.float32), lib.ptr(ln, torch.int32), lib.ptr(f0), lib.ptr(vo), lib.ptr(ap),
                     lib.ptr(cm), B, L, T, self.win, self.hop, self.tau_min, self.tau_max, self.sample_rate, self.threshold,
                     int(self.log), lib.stream(x))
        feat_length = torch.tensor([self.feat_length(n) for n in lens], dtype=torch.int64).to(x.device)
        if pitch_track:
            f0 = f0.unsqueeze(-1)
        return (f0,) + tuple(t for t in (vo, ap, cm) if t is not None) + (feat_length,)
